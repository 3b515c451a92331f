"""CPU: include/sppark_amd_fri.h -- fold, reduce, domain -- compiles as plain C and C++; every product library exports
sppark_fri_reduce and all but libsppark_m31 the fold and the domain; every rejection arrives with an owned message before a
device is looked up; the Python wrappers reject bad shapes before they reach the library; and the kernels' resources from
the code objects' metadata: no private segment, work-groups of 256 lanes, LDS only in reduce."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
ELEM = (("gl64", 8, 32), ("bls12_381", 32, 32), ("bn254", 32, 28), ("bb31x4", 16, 27), ("bb31", 4, 27), ("m31", 4, None))
INVALID = -1                                               # negated hipErrorInvalidValue
NATURAL, BITREV = 0, 1


def _rejected(L, err, word=None):
    msg = ctypes.string_at(err.message) if err.message else b""
    if err.message:
        L.drop_error_message(err.message)
    assert err.code == INVALID and msg, (err.code, msg)
    if word is not None:
        assert word in msg, msg


def test_fri_header_is_plain_c_and_cxx(tmp_path):
    body = ('#include "sppark_amd_fri.h"\n'
            'int main(void) {\n'
            '  SppError (*fo)(size_t, void *, const void *, uint32_t, uint32_t, const void *, const void *, int, void *) = sppark_fri_fold;\n'
            '  SppError (*dm)(size_t, void *, uint32_t, const void *, int, const void *, void *) = sppark_fri_domain;\n'
            '  SppError (*rd)(size_t, void *, const void *, int, uint32_t, size_t, size_t, size_t, const void *, const void *, int, void *)'
            ' = sppark_fri_reduce;\n'
            '  return (fo == 0) + (dm == 0) + (rd == 0) + SPPARK_FRI_NATURAL + (SPPARK_FRI_BITREV == 0); }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        if shutil.which(cc) is None:
            pytest.skip(cc + " not available")
        src = tmp_path / ("t." + ext)
        src.write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", INC, str(src)])


def test_fri_symbols_exported(libs):
    assert len(libs) == 11
    for name, path in libs.items():
        L = ctypes.CDLL(path)
        assert hasattr(L, "sppark_fri_reduce"), name
        for fn in ("sppark_fri_fold", "sppark_fri_domain"):
            assert hasattr(L, fn) == (name != "m31"), (name, fn)


def test_fri_calls_reject_bad_arguments_before_the_device(libs):
    from sppark_amd import ffi
    for name, eb, adicity in ELEM:
        L = ffi.load(name)
        lg = 4
        n = 1 << lg
        pool = [np.ones(2 * n * eb, dtype=np.uint8) for _ in range(3)]
        a, o, w = (x.ctypes.data for x in pool)
        small = np.ones(8 * eb, dtype=np.uint8)
        r = small.ctypes.data
        zero = np.zeros(32, dtype=np.uint8)
        big = np.full(32, 0xff, dtype=np.uint8)

        # reduce: columns layout of 3 columns, n apart
        red = lambda out=o, inp=a, base=0, lg_n=lg, width=3, cs=n, ls=1, wt=r, sub=None: \
            L.sppark_fri_reduce(0, out, inp, base, lg_n, width, cs, ls, wt, sub, 0, None)       # noqa: E731
        _rejected(L, red(out=None)); _rejected(L, red(inp=None)); _rejected(L, red(wt=None))
        _rejected(L, red(lg_n=33), b"lg_n")
        _rejected(L, red(width=0), b"width")
        _rejected(L, red(base=2), b"in_base")
        if name != "bb31x4":
            _rejected(L, red(base=1), b"in_base")
        _rejected(L, red(cs=n - 1), b"strides"); _rejected(L, red(cs=2, ls=2), b"strides"); _rejected(L, red(cs=1, ls=2), b"strides")
        _rejected(L, red(width=1 << 62, cs=1 << 40), b"overflows"); _rejected(L, red(lg_n=32, width=1 << 40, cs=1 << 32), b"overflows")
        _rejected(L, red(inp=a + 1), b"misaligned")
        _rejected(L, red(out=a + 2 * n * eb), b"overlap"); _rejected(L, red(out=a - eb), b"overlap")      # out over the matrix
        _rejected(L, red(out=r - eb), b"overlap")                                                          # out over the weights
        _rejected(L, red(sub=o + 5 * eb), b"overlap")                                                      # sub inside out
        if name == "m31":
            continue

        # fold
        fold = lambda out=o, inp=a, lg_n=lg, a_=1, beta=r, shift=None, order=NATURAL: \
            L.sppark_fri_fold(0, out, inp, lg_n, a_, beta, shift, order, None)                  # noqa: E731
        _rejected(L, fold(out=None)); _rejected(L, fold(inp=None)); _rejected(L, fold(beta=None))
        _rejected(L, fold(lg_n=33), b"lg_n")
        if adicity < 32:
            _rejected(L, fold(lg_n=adicity + 1), b"2-adicity")
        for arity in (0, 4, 7):
            _rejected(L, fold(a_=arity), b"lg_arity")
        _rejected(L, fold(lg_n=2, a_=3), b"lg_arity"); _rejected(L, fold(lg_n=0, a_=1), b"lg_arity")
        for order in (-1, 2):
            _rejected(L, fold(order=order), b"order")
        for order in (NATURAL, BITREV):
            for arity in (1, 2, 3):
                m = n >> arity
                for off in (eb, (m - 1) * eb, (n - 1) * eb, -eb, -(m - 1) * eb):             # out partly over in
                    _rejected(L, fold(out=a + off, a_=arity, order=order), b"overlap")
            _rejected(L, fold(beta=o + 3 * eb, order=order), b"overlap")                       # beta inside out
        _rejected(L, fold(out=a, order=BITREV), b"overlap")                                    # in place: NATURAL only
        _rejected(L, fold(shift=zero.ctypes.data), b"shift")
        if eb != 32:                                                                            # a word of ones is not canonical
            _rejected(L, fold(shift=big.ctypes.data), b"shift")

        # domain
        dom = lambda out=o, lg_n=lg, shift=None, order=NATURAL, z=None: L.sppark_fri_domain(0, out, lg_n, shift, order, z, None)   # noqa: E731
        _rejected(L, dom(out=None))
        _rejected(L, dom(lg_n=33), b"lg_n")
        if adicity < 32:
            _rejected(L, dom(lg_n=adicity + 1), b"2-adicity")
        _rejected(L, dom(order=2), b"order")
        _rejected(L, dom(z=o + 2 * eb), b"overlap")                                            # z inside out
        _rejected(L, dom(shift=zero.ctypes.data), b"shift")
        assert all((x == 1).all() for x in pool) and (small == 1).all()


def test_fri_wrappers_reject_bad_shapes(libs):
    from sppark_amd import fri
    x16, x8, x4, x6, k1, k2 = (np.ones(k, dtype=np.uint64) for k in (16, 8, 4, 6, 1, 2))
    with pytest.raises(ValueError, match="m31"):
        fri.fold(np.ones(4, dtype=np.uint32), np.ones(8, dtype=np.uint32), np.ones(1, dtype=np.uint32), field="m31")
    with pytest.raises(ValueError, match="m31"):
        fri.domain(np.ones(8, dtype=np.uint32), field="m31")
    for args, kw in (((x16[:8], x8, k1), {}), ((x4, x6, k1), {}), ((x4, x8, k2), {}), ((x4, x8, k1), dict(lg_arity=2)),
                     ((x4, x8, k1), dict(lg_arity=0)), ((x4, x8, k1), dict(lg_arity=4)), ((k1, x4, k1), dict(lg_arity=3)),
                     ((x4, x8, k1), dict(order=2)), ((x8, x8[:8], k1), dict(order=fri.BITREV)), ((x4, x8, k1), dict(shift="left")),
                     ((x4, x8, k1), dict(shift=k2))):
        with pytest.raises(ValueError):
            fri.fold(*args, field="gl64", **kw)
    for args, kw in (((x6,), {}), ((x8,), dict(order=5)), ((x8,), dict(z=k2))):
        with pytest.raises(ValueError):
            fri.domain(*args, field="gl64", **kw)
    mat = np.ones((3, 8), dtype=np.uint64)
    for args, kw in (((x4, mat, x4[:3]), {}), ((x8, mat, x4), {}), ((x8, mat, x4[:3]), dict(sub=k2)), ((x8, mat, x4[:3]), dict(base=True)),
                     ((x8, mat, x4[:3]), dict(layout="diagonal")), ((x8, np.ones((3, 6), dtype=np.uint64), x4[:3]), {})):
        with pytest.raises(ValueError):
            fri.reduce(*args, field="gl64", **kw)
    with pytest.raises(ValueError):
        fri.deep_quotient(x8, mat, x4[:3], k1, k1, lg_n=4, field="gl64")


KERNEL_OBJECTS = ["gl64__api_ntt_api.hip.o", "bb31__api_ntt_api.hip.o", "m31__api_poly_only_api.hip.o", "bb31x4__api_poly_only_api.hip.o",
                  "bls12_381__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o", "bn254__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o"]


@pytest.mark.parametrize("obj", KERNEL_OBJECTS)
def test_fri_kernels_resources(libs, obj):
    """Instances: fold 3 arities x 2 orders, domain 2 orders, reduce 2 layouts (bb31x4: twice, its own field and bb31) -- and,
    where an element is below 16 bytes, each twice: with 16-byte accesses and element-wise."""
    import isa_stats
    path = os.path.join(OBJ, obj)
    assert os.path.exists(path), path
    meta = isa_stats.metadata(isa_stats.code_object(path))
    hit = {k: v for k, v in meta.items() if "k_fri_" in k and "vgpr_count" in v}
    count = lambda word: len([k for k in hit if word in k])                                 # noqa: E731
    two = 1 if ("bb31x4" in obj or "WITH_MSM" in obj) else 2
    if "m31" in obj:
        assert count("k_fri_fold") == 0 and count("k_fri_domain") == 0 and count("k_fri_reduce") == 4, sorted(hit)
    else:
        assert count("k_fri_fold") == 6 * two and count("k_fri_domain") == 2 * two, sorted(hit)
        assert count("k_fri_reduce") == (2 + 4 if "bb31x4" in obj else 2 * two), sorted(hit)
    for name, md in hit.items():
        assert int(md.get("private_segment_fixed_size") or 0) == 0, (name, md)
        assert int(md.get("max_flat_workgroup_size") or 0) == 256, (name, md)
        if "k_fri_reduce" not in name:
            assert int(md.get("group_segment_fixed_size") or 0) == 0, (name, md)
