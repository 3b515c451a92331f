"""CPU: the route of the FRI calls (csrc/fri/fri_route.hpp make_fri_route, through tests/emu/emu_fri.cpp) as data: grid,
tile and access style for every element size, operation, arity and size."""
import ctypes

import pytest

from test_emulation_fri import CHUNK, FRI_T, emu

FOLD, DOMAIN, REDUCE = 0, 1, 2
NT, WG_PER_CU = 256, 8
KEYS = ("invalid", "grid", "block", "pack", "acc", "out_lg", "tile_bits", "grid_lg", "tiles", "chunks", "vec")


def route(elem_bytes, lg_n, cus, op, lg_arity=1, order=0, layout=0, width=1, aligned16=1):
    L = emu("gl64")                                         # (the route is the same function in every build)
    call = (ctypes.c_uint64 * 9)(elem_bytes, lg_n, cus, op, lg_arity, order, layout, width, aligned16)
    out = (ctypes.c_uint64 * 11)()
    L.emu_fri_route(call, out)
    return dict(zip(KEYS, [int(v) for v in out]))


@pytest.mark.parametrize("es", [4, 8, 16, 32])
def test_fold_and_domain_geometry(es):
    T = {4: 12, 8: 11, 16: 10, 32: 9}[es]
    assert T in FRI_T.values()
    pack = max(16 // es, 1)
    for cus in (1, 3, 256):
        for op, arities in ((FOLD, (1, 2, 3)), (DOMAIN, (0,))):
            for a in arities:
                for lg in range(a, 27):
                    for al in (1, 0):
                        r = route(es, lg, cus, op, lg_arity=a, aligned16=al)
                        assert not r["invalid"] and r["block"] == NT
                        lg_m = lg - a
                        vec = es >= 16 or (al and (1 << lg_m) >= pack)
                        assert r["vec"] == vec and r["pack"] == (pack if vec else 1)
                        # 64 bytes of inputs per lane and tile wherever that leaves a whole access of results
                        assert r["acc"] == max(((1 << T) // NT >> a) // r["pack"], 1)
                        assert 1 << r["out_lg"] == NT * r["acc"] * r["pack"]
                        if a == 1 and vec:
                            assert r["out_lg"] + 1 == T
                        assert r["tiles"] == 1 << r["tile_bits"] == max(1 << lg_m >> r["out_lg"], 1)
                        # the grid: a power of two that divides the tiles, the largest within the cap
                        g = r["grid"]
                        assert g == 1 << r["grid_lg"] and r["tiles"] % g == 0 and g <= cus * WG_PER_CU
                        assert g == r["tiles"] or 2 * g > cus * WG_PER_CU


def test_reduce_geometry():
    for es in (4, 8, 16, 32):
        pack = max(16 // es, 1)
        for layout in (0, 1):
            for lg in (0, 1, 2, 5, 12, 22):
                for width in (1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK):
                    for al in (1, 0):
                        r = route(es, lg, 256, REDUCE, layout=layout, width=width, aligned16=al)
                        assert not r["invalid"] and r["chunks"] == -(-width // CHUNK)
                        cols_vec = layout == 0 and (es >= 16 or al) and (1 << lg) >= pack
                        assert r["pack"] == (pack if cols_vec else 1)
                        assert r["vec"] == (es >= 16 or (bool(al) and (layout == 1 or cols_vec)))
                        assert r["grid"] == min(max((1 << lg) // (NT * r["pack"]), 1), 256 * WG_PER_CU)


def test_rejections():
    assert route(12, 5, 1, FOLD)["invalid"] and route(8, 33, 1, FOLD)["invalid"] and route(8, 5, 1, 3)["invalid"]
    assert route(8, 5, 1, FOLD, lg_arity=0)["invalid"] and route(8, 5, 1, FOLD, lg_arity=4)["invalid"]
    assert route(8, 2, 1, FOLD, lg_arity=3)["invalid"] and route(8, 5, 1, FOLD, order=2)["invalid"]
    assert route(8, 5, 1, REDUCE, width=0)["invalid"] and route(8, 5, 1, REDUCE, layout=2)["invalid"]
