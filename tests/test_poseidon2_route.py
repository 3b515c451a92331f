"""CPU: the route of a Poseidon2 call (sppark_amd/csrc/poseidon2/poseidon2_route.hpp make_poseidon2_route, read through
tests/emu/emu_poseidon2.cpp).  The steps are asserted literally at lg_n = 0, 10, 11, 10 + S + 1 and 28; for every lg_n
0 .. 28 every layer is written by exactly one step, a step reads only a layer written before it, and the grids are at
least one work-group and within the cap; a permutation is one launch; what the route cannot serve is invalid."""
import ctypes

import pytest

from test_emulation_poseidon2 import emu

PERMUTE, LEAVES, NODES, TOP = range(4)
OP_PERMUTE, OP_COMMIT = 0, 1
STEP = ("kernel", "grid", "block", "first", "lo", "hi", "fused", "items")
WG_PER_CU, NT, S, TOP_LG = 8, 256, 3, 10
CU_COUNTS = (1, 3, 256, 304)


def route(L, op=OP_COMMIT, es=4, rf=8, rp=13, count=0, lg=0, width=1, layout=0, cus=256):
    call = (ctypes.c_uint64 * 9)(op, es, rf, rp, count, lg, width, layout, cus)
    out = (ctypes.c_uint64 * 128)()
    n = L.emu_p2_route(call, out, 128)
    assert n >= 2
    head = dict(zip(("nsteps", "invalid"), out[:2]))
    steps = [dict(zip(STEP, out[2 + 8 * i: 10 + 8 * i])) for i in range(head["nsteps"])]
    return head, steps


def step(kernel, grid, first, lo, hi, items):
    return dict(kernel=kernel, grid=grid, block=NT, first=first, lo=lo, hi=hi, fused=hi + 1 - lo, items=items)


def test_constants():
    L = emu()
    assert (L.emu_p2_top(), L.emu_p2_fused(), L.emu_p2_wg_per_cu()) == (1 << TOP_LG, S, WG_PER_CU)


@pytest.mark.parametrize("es", (4, 8))
def test_literal_routes(es):
    L = emu()
    cap = 256 * WG_PER_CU
    r = lambda lg: route(L, es=es, lg=lg, width=5, cus=256)                               # noqa: E731
    head, steps = r(0)
    assert not head["invalid"] and steps == [step(LEAVES, 1, 0, 0, 0, 1), step(TOP, 1, 0, 1, 0, 1)]
    assert steps[1]["fused"] == 0                                                        # a single digest: the top only copies the root
    assert r(10)[1] == [step(LEAVES, 4, 0, 0, 0, 1024), step(TOP, 1, 0, 1, 10, 1024)]
    assert r(11)[1] == [step(LEAVES, 8, 0, 0, 0, 2048), step(NODES, 1, 0, 1, 3, 256), step(TOP, 1, 3, 4, 11, 256)]
    assert r(10 + S)[1] == [step(LEAVES, 32, 0, 0, 0, 8192), step(NODES, 4, 0, 1, 3, 1024), step(TOP, 1, 3, 4, 13, 1024)]
    assert r(10 + S + 1)[1] == [step(LEAVES, 64, 0, 0, 0, 1 << 14), step(NODES, 8, 0, 1, 3, 2048), step(NODES, 1, 3, 4, 6, 256),
                                step(TOP, 1, 6, 7, 14, 256)]
    want = [step(LEAVES, cap, 0, 0, 0, 1 << 28)]
    for k in range(6):                                                                   # layers 0, 3, .., 15 feed a nodes launch
        lanes = 1 << (28 - 3 * k - 3)
        want.append(step(NODES, min(cap, lanes // NT), 3 * k, 3 * k + 1, 3 * k + 3, lanes))
    want.append(step(TOP, 1, 18, 19, 28, 1024))
    assert r(28)[1] == want and want[6]["grid"] == 4 and want[1]["grid"] == cap


@pytest.mark.parametrize("es", (4, 8))
@pytest.mark.parametrize("lg", range(0, 29))
def test_commit_route_covers_every_layer_once_within_the_caps(es, lg):
    L = emu()
    for cus in CU_COUNTS:
        for width in (1, 9, 1000):
            for layout in (0, 1):
                head, steps = route(L, es=es, lg=lg, width=width, layout=layout, cus=cus)
                assert not head["invalid"] and len(steps) == 2 + max(0, -(-(lg - TOP_LG) // S))
                written = []
                for k, s in enumerate(steps):
                    assert s["block"] == NT and 1 <= s["grid"] <= cus * WG_PER_CU
                    assert s["fused"] == s["hi"] + 1 - s["lo"]
                    if s["kernel"] == LEAVES:
                        assert k == 0 and (s["lo"], s["hi"], s["items"]) == (0, 0, 1 << lg)
                    else:
                        assert s["first"] in written and s["lo"] == s["first"] + 1
                        if s["kernel"] == NODES:
                            assert s["hi"] == s["first"] + S <= lg and s["items"] == 1 << (lg - s["first"] - S)
                            assert (1 << (lg - s["first"])) > 1 << TOP_LG
                        else:
                            assert s["kernel"] == TOP and k == len(steps) - 1 and s["grid"] == 1
                            assert s["items"] == 1 << (lg - s["first"]) <= 1 << TOP_LG and s["hi"] == lg
                    if s["kernel"] != TOP:
                        assert s["grid"] == min(max(-(-s["items"] // NT), 1), cus * WG_PER_CU)
                    written += list(range(s["lo"], s["hi"] + 1))
                assert written == list(range(lg + 1))


def test_permute_route():
    L = emu()
    for es in (4, 8):
        for count, cus, grid in ((1, 256, 1), (256, 256, 1), (257, 256, 2), (1000, 1, 4), (1 << 20, 256, 2048), (1 << 20, 2, 16), (5, 0, 1)):
            head, steps = route(L, op=OP_PERMUTE, es=es, count=count, cus=cus)
            assert not head["invalid"] and steps == [step(PERMUTE, grid, 0, 1, 0, count)], (count, cus)


def test_invalid_routes():
    L = emu()
    bad = [dict(es=3), dict(es=16), dict(es=32), dict(lg=29), dict(width=0), dict(width=1 << 30), dict(es=8, width=1 << 29), dict(layout=2),
           dict(rf=0), dict(rf=1), dict(rf=7), dict(rf=18), dict(rp=65), dict(op=2), dict(op=OP_PERMUTE, count=0),
           dict(op=OP_PERMUTE, count=1 << 58)]
    for kw in bad:
        head, steps = route(L, **kw)
        assert head["invalid"] and not steps, kw
    for kw in (dict(rf=2, rp=0), dict(rf=16, rp=64), dict(width=(1 << 30) - 1), dict(cus=0), dict(op=OP_PERMUTE, count=(1 << 58) - 1)):
        assert not route(L, **kw)[0]["invalid"], kw
