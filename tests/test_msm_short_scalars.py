"""CPU: MSM over short scalars (include/sppark_amd_short.h) without a GPU.

  * the per-work-item body of k_breakdown_short (csrc/msm/msm_kernels.hpp), compiled for the host by
    tests/emu/emu_short_scalars.cpp: for every declared bit length 1 .. NBITS - 2, every legal stride, every window count
    a plan can have (1 .. ceil((b + 1) / 2), longest window within make_plan's 24 bits) and random / all-ones /
    single-top-bit scalars, sum_w +-d_w 2^off_w == s mod 2^b, |d_w| <= 2^(len_w - 1), and no window group changes a digit;
  * the route (csrc/msm/msm_route.hpp) with the short bound never overflows, sizes the piece tree so that a uniform short
    input fits it at every cell of the GPU test's grid, and with the full-width bound is the route of
    tests/emu/emu_plan.cpp -- the one the driver took before short scalars existed -- field by field;
  * the Python layer's argument handling: stride defaults, npoints from the stride, refusals before a library is loaded.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_plan import FIELD_G1, FIELD_G2, FIELD_WIRE, HEAD, KEYS, STEP, TUN, KERNELS, BUFS, FLAGS, check_route, plan_lib, plan_tuned, route   # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FEATURES = [("BLS12_381", 255), ("BN254", 254), ("BLS12_377", 253)]
# the GPU test's grid (tests/test_msm_short_scalars_gpu.py)
GRID_N = (1, 255, (1 << 10) + 3, (1 << 14) + 7, (1 << 17) + 1, 1 << 18)
GRID_B = lambda nbits: (1, 8, 31, 32, 33, 64, 65, 128, 129, nbits - 2)        # noqa: E731
RESIDENT = 2 * 256 * 256                    # lanes of k_accumulate an MI355X holds (tests/test_msm_route.py)


def _emu(feature):
    so = os.path.join(EMU, "libemu_short_scalars_%s.so" % feature)
    src = os.path.join(EMU, "emu_short_scalars.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max(os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs)
    newest = max(newest, os.stat(src).st_mtime)
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-DFEATURE_" + feature, "-o", so, src])
    L = ctypes.CDLL(so)
    cu, up, u64 = ctypes.c_uint, ctypes.POINTER(ctypes.c_uint), ctypes.c_uint64
    L.emu_short_cell.argtypes = [cu, cu, cu, cu, u64]
    L.emu_short_sweep.argtypes = [u64, up, up]
    L.emu_short_sweep.restype = ctypes.c_ulong
    L.emu_short_route.argtypes = [ctypes.c_size_t, cu, up, ctypes.c_size_t, up, up, cu, up, up, cu]
    L.emu_short_route.restype = cu
    L.emu_short_max_pieces.argtypes = [cu, cu, cu, cu, u64]
    L.emu_short_max_pieces.restype = cu
    return L


@pytest.fixture(scope="module", params=FEATURES, ids=[f for f, _ in FEATURES])
def emu(request):
    feature, nbits = request.param
    L = _emu(feature)
    assert L.emu_short_nbits() == nbits
    return L, nbits


def _uints(v):
    return (ctypes.c_uint * len(v))(*v)


def short_route(L, n, plan_bits, field, short_bits, resident=RESIDENT, fb_n=0, redo=0, may_defer=0, convert=0, flagged=0, stride=0,
                aligned16=1, top_cut=0, **tun):
    """(plan, head, steps) of make_plan(n, plan_bits) and make_route with msm_call::short_bits, decoded as test_plan.route does"""
    plan, out = (ctypes.c_uint * 21)(), (ctypes.c_uint * 4096)()
    nw = L.emu_short_route(n, plan_bits, _uints([tun.get(k, 0) for k in TUN]), resident, _uints(field),
                           _uints([fb_n, redo, may_defer, convert, flagged, stride, aligned16, top_cut]), short_bits, plan, out, 4096)
    assert nw, (n, plan_bits, tun)
    head = dict(zip(HEAD, out[:11]))
    head["result"] = BUFS[head["result"]]
    steps = []
    for i in range(head["nsteps"]):
        d = dict(zip(STEP, out[11 + 20 * i:31 + 20 * i]))
        d["kernel"] = KERNELS[d["kernel"]]; d["flag"] = FLAGS[d["flag"]]
        for k in ("rd0", "rd1", "wr0", "wr1"):
            d[k] = BUFS[d[k]]
        steps.append(d)
    return dict(zip(KEYS, plan)), head, steps


def _sizes():
    """the sizes of tests/test_plan.py's ladder: every power of two up to 2^31 with its neighbours"""
    ns = set()
    for lg in range(0, 32):
        ns.update({1 << lg, (1 << lg) + 1, (1 << lg) * 3 // 2 + 7, max(1, (1 << lg) - 1)})
    return sorted(n for n in ns if n <= 1 << 31)


def test_breakdown_short_body(emu):
    """every bit length x stride x window count x scalar kind through the kernel's own body (a few seconds per field)"""
    L, nbits = emu
    failed, first = ctypes.c_uint(0), (ctypes.c_uint * 5)()
    cells = L.emu_short_sweep(0x5eed, ctypes.byref(failed), first)
    assert cells > 100000
    assert failed.value == 0, "first failure: bits %d stride %d windows %d kind %d code %d" % tuple(first)
    # the check itself sees a wrong digit run: a stride the loads must not exceed is covered by the exact allocations of the
    # harness under a sanitizer (the stand-alone build); here: the cells are not vacuous -- the digits of 2^b - 1 are not all zero
    assert L.emu_short_cell(64, 8, 3, 1, 1) == 0 and L.emu_short_cell(nbits - 2, 32, 12, 2, 1) == 0


def test_short_route_never_overflows(emu):
    """the route of a short call at every ladder size x the grid's bit lengths x the three field kinds, first pass (alone /
    one of several chunks) and second pass, one or three window groups: a valid route, never an overflow"""
    L, nbits = emu
    for n in _sizes():
        for b in GRID_B(nbits):
            for field in (FIELD_G1, FIELD_G2, FIELD_WIRE):
                for groups in (0, 3):
                    tun = dict(groups=groups, long_runs=int(field is FIELD_G2))
                    for redo, may_defer in ((0, 1), (0, 0), (1, 0)):
                        p, head, steps = short_route(L, n, b + 1, field, b, redo=redo, may_defer=may_defer, convert=field[0],
                                                     flagged=n & 1, stride=2 * field[6] + 8 * (n & 1), **tun)
                        why = (n, b, field, groups, redo, may_defer)
                        assert p["nbits"] == b + 1 and p["nwins"] == -(-(b + 1) // p["wbits"]), why
                        check_route(p, field, head, steps, why)
                        assert redo or may_defer or not head["pieces"], why


def test_full_width_route_is_unchanged(emu, plan_lib):
    """short_bits = 0: plan and route are those of tests/emu/emu_plan.cpp (which knows nothing of short scalars and builds its
    msm_call with the defaults), field by field, at every ladder size"""
    L, nbits = emu
    for n in _sizes():
        for field in (FIELD_G1, FIELD_G2, FIELD_WIRE):
            for groups in (0, 3):
                tun = dict(groups=groups, long_runs=int(field is FIELD_G2))
                want_p = plan_tuned(plan_lib, n, nbits, RESIDENT, **tun)
                for redo, may_defer in ((0, 1), (0, 0), (1, 0)):
                    call = dict(redo=redo, may_defer=may_defer, convert=field[0], flagged=n & 1, stride=2 * field[6] + 8 * (n & 1))
                    p, head, steps = short_route(L, n, nbits, field, 0, **call, **tun)
                    assert p == want_p, (n, field, groups)
                    assert (head, steps) == route(plan_lib, want_p, field, nbits, **call, **tun), (n, field, groups, redo, may_defer)


def test_uniform_short_input_fits_the_piece_tree(emu):
    """The GPU test asserts that tail_redone() does not move over the uniform cells of its grid.  That is satisfiable: at every
    cell the fullest bucket of a uniform b-bit input -- counted through the kernel's body -- is within the pieces the route
    sizes the piece tree for (and where the route sizes none, there is no piece tree to overflow)."""
    L, nbits = emu
    sized = 0
    for n in GRID_N:
        for b in GRID_B(nbits):
            p, head, _ = short_route(L, n, b + 1, FIELD_G1, b, may_defer=1, convert=1, stride=2 * FIELD_G1[6])
            if not head["piece_cmax"]:
                continue
            sized += 1
            worst = L.emu_short_max_pieces(n, b, p["nwins"], p["L"], 0xabc + n + b)
            assert worst <= head["piece_cmax"], (n, b, p, worst, head["piece_cmax"])
    assert sized >= 10


# ---- the Python layer ---------------------------------------------------------------------------------------------------
def test_python_stride_defaults_and_refusals(monkeypatch):
    from sppark_amd import ffi, msm

    def no_load(*a, **k):
        raise AssertionError("a refused call must not load a library")
    monkeypatch.setattr(ffi, "load", no_load)
    form = msm.short_scalar_form
    assert form(np.zeros(5, dtype=np.uint64), 64) == (64, 8)
    assert form(np.zeros(5, dtype=np.uint32), 31) == (31, 4)
    assert form(np.zeros((5, 12), dtype=np.uint8), 65) == (65, 12)
    assert form(np.zeros((5, 2), dtype=np.uint64), 128) == (128, 16)
    assert form(np.zeros((5, 4), dtype=np.uint64), 64) == (64, 32)            # short values in wide slots
    assert form(np.zeros(40, dtype=np.uint8), 64, 8) == (64, 8)
    assert form(np.zeros(40, dtype=np.uint8), 253, 32, "bls12_381") == (253, 32)
    try:
        import torch
        assert form(torch.zeros(5, dtype=torch.uint64), 40) == (40, 8)
        assert form(torch.zeros((5, 5), dtype=torch.int32), 129) == (129, 20)
    except (ImportError, AttributeError):
        pass
    pts = np.zeros((5, 104), dtype=np.uint8)
    for bad in (dict(scalar_bits=0), dict(scalar_bits=254), dict(scalar_bits=33, scalar_stride=4), dict(scalar_bits=8, scalar_stride=6),
                dict(scalar_bits=8, scalar_stride=36), dict(scalar_bits=-1)):
        with pytest.raises(ValueError):
            msm.multi_scalar_mult_arkworks(pts, np.zeros((5, 8), dtype=np.uint8), "bls12_381", **bad)
        with pytest.raises(ValueError):
            msm.multi_scalar_mult_fp2_arkworks(np.zeros((5, 200), dtype=np.uint8), np.zeros((5, 8), dtype=np.uint8), "bls12_381", **bad)
    with pytest.raises(ValueError):         # a 1-D byte array says nothing about the stride
        msm.multi_scalar_mult_arkworks(pts, np.zeros(40, dtype=np.uint8), "bls12_381", scalar_bits=64)
    with pytest.raises(ValueError):         # bn254: NBITS - 2 = 252
        form(np.zeros((5, 32), dtype=np.uint8), 253, None, "bn254")


class _FakeLib:
    """records the short-scalar calls the Python layer makes"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return type("E", (), {"code": 0, "message": None})()
        return fn


def test_python_npoints_from_the_stride(monkeypatch):
    from sppark_amd import ffi, msm
    fake = _FakeLib()
    monkeypatch.setattr(ffi, "load", lambda name: fake)
    ctx = msm.MsmContext("bls12_381")
    sc = np.zeros(7, dtype=np.uint64)
    ctx.invoke(None, sc, scalar_bits=64)                                    # preloaded bases: n from the scalars, by the stride
    name, a = fake.calls[-1]
    assert name == "sppark_msm_invoke_bits" and a[3] == 7 and a[5:7] == (64, 8)
    ctx.invoke(None, np.zeros((7, 16), dtype=np.uint8), scalar_bits=64)
    assert fake.calls[-1][1][3] == 7 and fake.calls[-1][1][5:7] == (64, 16)
    ctx.invoke(None, np.zeros((7, 32), dtype=np.uint8))                      # without scalar_bits nothing changes
    name, a = fake.calls[-1]
    assert name == "sppark_msm_invoke" and a[3] == 7
    pts = np.zeros((7, 104), dtype=np.uint8)
    msm.multi_scalar_mult_arkworks(pts, sc, "bls12_381", scalar_bits=33)
    name, a = fake.calls[-1]
    assert name == "mult_pippenger_inf_bits" and a[2] == 7 and a[4:] == (33, 8, 104)
    with pytest.raises(ValueError):                                          # 7 points, 6 scalars
        msm.multi_scalar_mult_arkworks(pts, sc[:6], "bls12_381", scalar_bits=33)
    with pytest.raises(ValueError):                                          # a base that is not aligned to its 8-byte stride
        ctx.invoke(None, np.zeros(60, dtype=np.uint8)[4:], scalar_bits=64, scalar_stride=8)
    ctx.reserve(1 << 10, 104, scalar_bits=64)
    assert fake.calls[-1] == ("sppark_msm_reserve_bits", (ctx.h, 1 << 10, 104, 0, 0, 64, 8))
    ctx.plan(1 << 10, scalar_bits=64)
    assert fake.calls[-1][0] == "sppark_msm_plan_bits" and fake.calls[-1][1][1:3] == (1 << 10, 64)
    with pytest.raises(ValueError):
        ctx.invoke(None, sc, scalar_bits=64, mont=True)
    ctx.h = None
