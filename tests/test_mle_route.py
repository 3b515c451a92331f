"""CPU: the route of the multilinear-table calls (sppark_amd/csrc/mle/mle_route.hpp make_mle_route, read through
tests/emu/emu_mle.cpp) for lg_n = 0 .. 32 and the four element sizes: the variables bound add up to lg_n, every grid is at
least one work-group and within the cap, the scratch is what the launches write, launch counts never fall as lg_n grows."""
import ctypes

import pytest

from test_emulation_mle import emu

FOLD, EVALUATE, EQ, ROUND = 0, 1, 2, 3
MK_FOLD, MK_BIND, MK_EQ, MK_ROUND, MK_ROUND_SUM = range(5)
STEP = ("kernel", "grid", "block", "tile_lg", "vars", "var_base", "tiles", "writes", "vec")
TILE_LG = {4: 12, 8: 11, 16: 10, 32: 9}            # mle_route.hpp mle_tile_lg
WG_PER_CU = 8                                      # mle_route.hpp MLE_WG_PER_CU
CU_COUNTS = (1, 3, 256, 304)


def route(L, es, lg, cus, op, rows=0, aligned=1):
    call = (ctypes.c_uint64 * 6)(es, lg, cus, op, rows, aligned)
    out = (ctypes.c_uint64 * 128)()
    n = L.emu_mle_route(call, out, 128)
    assert n >= 3
    head = dict(zip(("nsteps", "invalid", "scratch_elems"), out[:3]))
    steps = [dict(zip(STEP, out[3 + 9 * i: 12 + 9 * i])) for i in range(head["nsteps"])]
    return head, steps


@pytest.fixture(scope="module")
def L():
    return emu("gl64")


def _common(head, steps, cus):
    assert not head["invalid"]
    for s in steps:
        assert s["block"] == 256
        assert 1 <= s["grid"] <= cus * WG_PER_CU
        assert s["grid"] <= max(s["tiles"], 1)
    assert head["scratch_elems"] == sum(s["writes"] for s in steps)


@pytest.mark.parametrize("es", sorted(TILE_LG))
@pytest.mark.parametrize("lg", range(0, 33))
def test_evaluate_and_eq_routes(L, es, lg):
    T = TILE_LG[es]
    for cus in CU_COUNTS:
        for aligned in (0, 1):
            head, steps = route(L, es, lg, cus, EVALUATE, aligned=aligned)
            _common(head, steps, cus)
            assert len(steps) == -(-lg // T)
            assert all(s["kernel"] == MK_BIND for s in steps)
            assert sum(s["vars"] for s in steps) == lg
            left = lg
            for i, s in enumerate(steps):
                assert s["var_base"] == lg - left and s["vars"] == s["tile_lg"] <= T
                left -= s["vars"]
                assert s["tiles"] == 1 << left == s["writes"]              # one element per tile, the last pass one in all
                if es < 16:                                                 # 16-byte accesses: whole tiles from aligned memory only
                    assert s["vec"] == (s["tile_lg"] == T and (i > 0 or aligned == 1))
            assert left == 0
            head, steps = route(L, es, lg, cus, EQ, aligned=aligned)
            _common(head, steps, cus)
            assert len(steps) == 1 and steps[0]["kernel"] == MK_EQ
            s = steps[0]
            assert s["vars"] == lg and s["tile_lg"] == min(lg, T) and s["tiles"] == 1 << (lg - s["tile_lg"]) and s["writes"] == 0
            if es < 16:
                assert s["vec"] == (aligned == 1 and lg >= T)


@pytest.mark.parametrize("es", sorted(TILE_LG))
@pytest.mark.parametrize("lg", range(1, 33))
def test_fold_and_round_routes(L, es, lg):
    T = TILE_LG[es]
    for cus in CU_COUNTS:
        for aligned in (0, 1):
            head, steps = route(L, es, lg, cus, FOLD, aligned=aligned)
            _common(head, steps, cus)
            assert len(steps) == 1 and steps[0]["kernel"] == MK_FOLD
            s = steps[0]
            assert s["vars"] == 1 and s["writes"] == 0 and s["tiles"] == max(1, 1 << max(lg - T, 0))
            if es < 16:                                                     # n / 2 results fill at least one 16-byte access
                assert s["vec"] == (aligned == 1 and (1 << (lg - 1)) * es >= 16)
            for rows in (2, 3, 4, 5):
                head, steps = route(L, es, lg, cus, ROUND, rows=rows, aligned=aligned)
                _common(head, steps, cus)
                assert [s["kernel"] for s in steps] == [MK_ROUND, MK_ROUND_SUM]
                assert steps[0]["writes"] == steps[0]["grid"] * rows           # one slab row per work-group
                assert steps[1]["grid"] == 1 and steps[1]["tiles"] == steps[0]["grid"] and steps[1]["writes"] == rows
                assert sum(s["vars"] for s in steps) == 0


@pytest.mark.parametrize("es", sorted(TILE_LG))
def test_launch_counts_are_monotone(L, es):
    for op, lo in ((FOLD, 1), (EVALUATE, 0), (EQ, 0), (ROUND, 1)):
        counts = [route(L, es, lg, 256, op, rows=4)[0]["nsteps"] for lg in range(lo, 33)]
        assert counts == sorted(counts), (es, op)
    changes = [lg for lg in range(1, 33) if route(L, es, lg, 256, EVALUATE)[0]["nsteps"] != route(L, es, lg - 1, 256, EVALUATE)[0]["nsteps"]]
    assert changes == [1, TILE_LG[es] + 1, 2 * TILE_LG[es] + 1] + ([3 * TILE_LG[es] + 1] if 3 * TILE_LG[es] < 32 else [])


def test_rejected_calls(L):
    for es, lg, op, rows in ((8, 33, EVALUATE, 0), (8, 0, FOLD, 0), (8, 0, ROUND, 4), (8, 4, ROUND, 1), (8, 4, ROUND, 6), (12, 4, EQ, 0),
                             (8, 4, 4, 0)):
        head, steps = route(L, es, lg, 256, op, rows=rows)
        assert head["invalid"] and not steps
