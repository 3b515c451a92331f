"""CPU: the route of a Merkle commitment (sppark_amd/csrc/merkle/merkle_route.hpp make_merkle_route, read through
tests/emu/emu_merkle.cpp) for lg_n = 0 .. 28, the four element sizes and widths 1, 16, 17 and 1000: every layer 0 .. lg_n is
written by exactly one step, a step reads only a layer written before it, grids are at least one work-group and within the
cap, the last step produces the root, and what the route cannot serve is invalid."""
import ctypes

import pytest

from test_emulation_merkle import emu

LEAVES, NODES, TOP = range(3)
STEP = ("kernel", "grid", "block", "first", "lo", "hi", "fused", "items")
WG_PER_CU = 8                                      # merkle_route.hpp MERKLE_WG_PER_CU
CU_COUNTS = (1, 3, 256, 304)
WIDTHS = (1, 16, 17, 1000)


def route(L, es, lg, width, layout, hash, cus):                                          # noqa: A002
    call = (ctypes.c_uint64 * 6)(es, lg, width, layout, hash, cus)
    out = (ctypes.c_uint64 * 128)()
    n = L.emu_merkle_route(call, out, 128)
    assert n >= 2
    head = dict(zip(("nsteps", "invalid"), out[:2]))
    steps = [dict(zip(STEP, out[2 + 8 * i: 10 + 8 * i])) for i in range(head["nsteps"])]
    return head, steps


@pytest.mark.parametrize("es", (4, 8, 16, 32))
@pytest.mark.parametrize("lg", range(0, 29))
def test_commit_route(es, lg):
    L = emu()
    top, fused = L.emu_merkle_top(), L.emu_merkle_fused()
    for cus in CU_COUNTS:
        for width in WIDTHS:
            for layout in (0, 1):
                for hash in (0, 1):                                                      # noqa: A001
                    head, steps = route(L, es, lg, width, layout, hash, cus)
                    assert not head["invalid"] and len(steps) >= 2
                    written = []
                    for k, s in enumerate(steps):
                        assert s["block"] == 256
                        assert 1 <= s["grid"] <= cus * WG_PER_CU
                        if s["kernel"] == LEAVES:
                            assert k == 0 and (s["lo"], s["hi"], s["items"]) == (0, 0, 1 << lg)
                            assert s["grid"] <= max(-(-s["items"] // 256), 1)
                        else:
                            assert s["first"] in written, (k, s)                          # reads only what an earlier step wrote
                            assert s["lo"] == s["first"] + 1
                            if s["kernel"] == NODES:
                                assert s["fused"] == fused and s["hi"] == s["first"] + fused <= lg
                                assert s["items"] == 1 << (lg - s["first"] - fused)       # 2^fused digests per lane
                                assert (1 << (lg - s["first"])) > top                    # only above the top kernel's reach
                                assert s["grid"] <= max(-(-s["items"] // 256), 1)
                            else:
                                assert s["kernel"] == TOP and k == len(steps) - 1 and s["grid"] == 1
                                assert s["items"] == 1 << (lg - s["first"]) <= top and s["hi"] == lg
                        written += list(range(s["lo"], s["hi"] + 1))
                        assert s["fused"] == s["hi"] + 1 - s["lo"]
                    assert written == list(range(lg + 1))                                # every layer once, bottom-up
                    assert steps[-1]["kernel"] == TOP and steps[-1]["hi"] == lg          # the root
                    assert len(steps) == 2 + max(0, -(-(lg - 10) // fused))


def test_node_launch_counts():
    L = emu()
    count = lambda lg: len([s for s in route(L, 4, lg, 1, 0, 0, 256)[1] if s["kernel"] == NODES])     # noqa: E731
    assert [count(lg) for lg in (0, 10, 11, 13, 14, 16, 17, 28)] == [0, 0, 1, 1, 2, 2, 3, 6]


def test_invalid_routes():
    L = emu()
    for call in ((3, 4, 1, 0, 0, 8), (64, 4, 1, 0, 0, 8), (4, 29, 1, 0, 0, 8), (4, 4, 0, 0, 0, 8), (4, 4, 1 << 30, 0, 0, 8),
                 (32, 4, 1 << 27, 0, 0, 8), (4, 4, 1, 2, 0, 8), (4, 4, 1, 0, 2, 8)):
        head, steps = route(L, *call)
        assert head["invalid"] and not steps, call
    assert not route(L, 4, 4, (1 << 30) - 1, 0, 0, 8)[0]["invalid"]
    assert not route(L, 4, 4, 1, 0, 0, 0)[0]["invalid"]                                  # (no CU count: one work-group per step)
