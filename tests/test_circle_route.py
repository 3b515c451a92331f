"""CPU: the circle transform's route (sppark_amd/csrc/circle/circle_route.hpp make_circle_route, read through
tests/emu/emu_circle.cpp) for every size the entry points accept: the layers add up, one step scales an inverse, the
LDS and grid caps hold, the launch count is the documented one, and no table request exceeds its cap."""
import ctypes

import pytest

from test_emulation_circle import emu

LOW, HIGH, CACHE_LG = 12, 8, 24                 # circle_knobs: layers of the lowest pass / of a pass above it; cached tables
CK_PASS = 0
STEP = ("kernel", "gx", "gy", "block", "lds", "lg", "b_lo", "S", "lgC", "lgT", "inverse", "scales", "vec", "pad_lg")


def route(L, lg, order, direction, batch, max_grid_y=65535, aligned=1, pad_lg=32):
    call = (ctypes.c_uint64 * 7)(lg, order, direction, batch, max_grid_y, aligned, pad_lg)
    out = (ctypes.c_uint64 * 1024)()
    n = L.emu_circle_route(call, out, 1024)
    assert n >= 6
    head = dict(zip(("nsteps", "ntables", "invalid", "cols", "scratch_entries", "needs_points"), out[:6]))
    steps = [dict(zip(STEP, out[6 + 14 * i: 20 + 14 * i])) for i in range(head["nsteps"])]
    t0 = 6 + 14 * head["nsteps"]
    tables = [dict(zip(("m", "y", "cached", "count"), out[t0 + 4 * i: t0 + 4 * i + 4])) for i in range(head["ntables"])]
    return head, steps, tables


def launches(lg):
    return 1 if lg <= LOW else 1 + -(-(lg - LOW) // HIGH)


@pytest.fixture(scope="module")
def L():
    lib = emu()
    lib.emu_circle_knobs(0, 0, 0, 0, 0)
    return lib


@pytest.mark.parametrize("lg", range(0, 31))
def test_route_every_size(L, lg):
    assert L.emu_circle_point_entries() <= 1 << 16
    for batch in (1, 2, 70000):
        for order in (0, 1):
            for direction in (0, 1):
                head, steps, tables = route(L, lg, order, direction, batch)
                assert not head["invalid"]
                if lg == 0:
                    assert head["nsteps"] == 0 and head["ntables"] == 0
                    continue
                passes = [s for s in steps if s["kernel"] == CK_PASS]
                assert len(passes) == launches(lg) and len(steps) == launches(lg) + (1 if order == 1 else 0)
                assert sum(s["S"] for s in passes) == lg
                # consecutive layers, top down forward, bottom up inverse; the bit reversal on the evaluations' side
                order_lo = [s["b_lo"] for s in passes]
                assert order_lo == sorted(order_lo, reverse=(direction == 0))
                covered = sorted((s["b_lo"], s["b_lo"] + s["S"]) for s in passes)
                assert covered[0][0] == 0 and all(a[1] == b[0] for a, b in zip(covered, covered[1:])) and covered[-1][1] == lg
                if order == 1:
                    assert steps[-1 if direction == 0 else 0]["kernel"] != CK_PASS
                assert sum(s["scales"] for s in steps) == (1 if direction == 1 else 0)
                if direction == 1:
                    assert passes[-1]["scales"]
                assert 1 <= head["cols"] <= batch
                for s in steps:
                    assert s["lds"] <= 65536 and 1 <= s["gy"] <= 65535 and s["gx"] >= 1 and s["block"] == 256
                    if s["kernel"] != CK_PASS:
                        assert s["gy"] == head["cols"]
                        continue
                    assert 1 <= s["S"] <= 12 and s["lgT"] <= 12 and s["lds"] == 4 * ((1 << s["lgT"]) + ((1 << s["lgT"]) >> 4) + (1 << s["S"]))
                    if s["b_lo"] == 0:
                        assert s["lgC"] == 0 and s["S"] == min(lg, LOW)
                        packed = s["lgT"] - s["S"]
                        assert (packed == 0 or lg < 12) and s["gx"] << s["S"] == 1 << lg
                        assert s["gy"] << packed >= head["cols"] > (s["gy"] - 1) << packed
                    else:
                        assert s["S"] <= HIGH and s["lgC"] >= 4 and s["lgT"] == s["S"] + s["lgC"] and s["lgC"] <= s["b_lo"]
                        assert s["gx"] << s["lgT"] == 1 << lg and s["gy"] == head["cols"]
                    assert s["pad_lg"] >= lg
                # tables: forward wants the 4096 points only; inverse one table per layer (none for the y-layer of lg = 1)
                if direction == 0:
                    assert head["needs_points"] and not tables and head["scratch_entries"] == 0
                else:
                    assert len(tables) == (lg if lg >= 2 else 0)
                    assert sorted((t["m"], t["y"]) for t in tables) == sorted([(lg, 1)] + [(m, 0) for m in range(2, lg + 1)]) if lg >= 2 else True
                    for t in tables:
                        assert t["count"] == 1 << (t["m"] - 2) and t["cached"] == (t["m"] <= CACHE_LG)
                    assert sum(t["count"] for t in tables if t["cached"]) * 4 <= 64 << 20
                    assert head["scratch_entries"] == sum(t["count"] for t in tables if not t["cached"]) <= 1 << lg


def test_route_batches_split_at_the_grid_limit(L):
    head, steps, _ = route(L, 2, 0, 0, 70000)
    assert head["cols"] == 70000 and steps[0]["gy"] == -(-70000 // 1024)        # 1024 columns of 2^2 share a work-group
    head, steps, _ = route(L, 2, 1, 0, 70000)
    assert head["cols"] == 65535                                                # the bit reversal takes a grid row per column
    head, steps, _ = route(L, 13, 0, 1, 70000)
    assert head["cols"] == 65535 and all(s["gy"] == 65535 for s in steps)
    head, steps, _ = route(L, 6, 0, 0, 3)
    assert steps[0]["lgT"] == 8 and steps[0]["gy"] == 1                         # 3 columns of 2^6: one work-group of 4 slots
    head, steps, _ = route(L, 14, 0, 0, 5, max_grid_y=2)
    assert head["cols"] == 2


def test_route_alignment_and_padding(L):
    for lg in (1, 2, 5, 12, 13, 21):
        _, steps, _ = route(L, lg, 1, 0, 3, aligned=0)
        assert not any(s["vec"] for s in steps if s["kernel"] == CK_PASS)
        assert all(s["kernel"] != 3 for s in steps)                             # no 16-byte bit reversal either
        _, steps, _ = route(L, lg, 0, 0, 3, aligned=1)
        assert all(s["vec"] == (lg >= 2) for s in steps)
    # the LDE's padding rides in the FIRST forward pass only; a source below four elements is read element-wise
    for lg, pad in ((14, 12), (22, 20), (5, 2), (3, 1), (3, 0)):
        _, steps, _ = route(L, lg, 0, 0, 2, pad_lg=pad)
        assert [s["pad_lg"] < lg for s in steps] == [True] + [False] * (len(steps) - 1)
        assert steps[0]["pad_lg"] == pad and steps[0]["vec"] == (pad >= 2)
    _, steps, _ = route(L, 14, 0, 1, 2, pad_lg=12)
    assert all(s["pad_lg"] >= 14 for s in steps)


def test_route_rejects_what_the_entry_points_reject(L):
    for lg, order, direction in ((31, 0, 0), (4, 2, 0), (4, 0, 2)):
        head, _, _ = route(L, lg, order, direction, 1)
        assert head["invalid"]
