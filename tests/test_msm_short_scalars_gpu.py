"""GPU: MSM over short scalars (include/sppark_amd_short.h; k_breakdown_short) against the unchanged full-width path.

The yardstick of every case is the same context's ordinary invoke on the same VALUES -- the low b bits of what the short
call was handed -- zero-extended to 32 bytes: the only way a caller could compute it before.  What the short call is handed
is random in every byte of its slot, so whatever lies above bit b (the rest of the top word, the rest of a wider slot) must be
masked by the kernel for the two to agree.  Results are compared after to_affine; up to 2^10 points also against the oracle.
Points are distinct (generate_points / generate_progression on the device)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NBITS = {"bls12_381": 255, "bn254": 254, "bls12_377": 253, "pallas": 255, "vesta": 255}
ORACLE_ID = {"bls12_381": 0, "bn254": 1, "bls12_377": 4, "pallas": 6, "vesta": 7}
GRID_N = [1, 255, (1 << 10) + 3, (1 << 14) + 7, (1 << 17) + 1, 1 << 18]
TOP = 1 << 18


def grid_b(name):
    return [(1, 4), (8, 4), (31, 4), (32, 4), (33, 8), (64, 8), (65, 12), (128, 16), (129, 20), (NBITS[name] - 2, 32)]


def masked32(raw, b):
    """(n, S) bytes -> (n, 32) bytes: the low b bits of every row, zero-extended"""
    n, S = raw.shape
    out = np.zeros((n, 32), dtype=np.uint8)
    nb = (b + 7) // 8
    out[:, :nb] = raw[:, :nb]
    if b % 8:
        out[:, nb - 1] &= (1 << (b % 8)) - 1
    return out


def random_slots(n, S, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, S), dtype=np.uint8)


_POINTS = {}


def points_of(name, fb):
    """2^18 distinct points k_i G of |name| (flagged 2 fb + 8 byte records): (host array, device tensor), made once"""
    import torch
    import sppark_amd
    if name not in _POINTS:
        host = np.zeros((TOP, 2 * fb + 8), dtype=np.uint8)
        sppark_amd.generate_points(host, TOP, 0x5107 + len(name), 2 * fb + 8, name)
        _POINTS[name] = (host, torch.from_numpy(host).cuda())
    return _POINTS[name]


def affine(out, name):
    import sppark_amd
    return sppark_amd.to_affine(out, name)


def check_cell(ctx, name, pts_dev, n, b, S, seed, oracle=None, pts_host=None, device_scalars=True):
    """short call == yardstick (== oracle); returns how often the tail ran twice during the SHORT call"""
    import torch
    raw = random_slots(n, S, seed)
    wide = masked32(raw, b)
    sc, sc32 = (torch.from_numpy(raw).cuda(), torch.from_numpy(wide).cuda()) if device_scalars else (raw, wide)
    stride = pts_dev.shape[1]
    before = ctx.tail_redone()
    got = affine(ctx.invoke(pts_dev[:n], sc, npoints=n, ffi_affine_sz=stride, scalar_bits=b, scalar_stride=S), name)
    redone = ctx.tail_redone() - before
    want = affine(ctx.invoke(pts_dev[:n], sc32, npoints=n, ffi_affine_sz=stride), name)
    assert (got == want).all(), (name, n, b, S)
    if oracle is not None:
        assert (got == oracle.msm_affine(ORACLE_ID[name], pts_host[:n], wide, algo=0, param=8)).all(), (name, n, b, S, "oracle")
    return redone


@pytest.mark.parametrize("n", GRID_N)
@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_short_parity_grid(oracle, libs, name, n):
    """n x (b, S): the short call, the yardstick and (n <= 2^10) the oracle agree; the plan has ceil((b + 1) / window) windows;
    uniform scalars never make the tail run twice (the piece tree is sized by the short bound, tests/test_msm_short_scalars.py)"""
    import sppark_amd
    fb = sppark_amd.msm.FP_BYTES[name]
    host, dev = points_of(name, fb)
    ctx = sppark_amd.MsmContext(name)
    for b, S in grid_b(name):
        p = ctx.plan(n, scalar_bits=b)
        assert p["windows"] == -(-(b + 1) // p["window_bits"]) and p["buckets_per_window"] == 1 << (p["window_bits"] - 1), (n, b, p)
        redone = check_cell(ctx, name, dev, n, b, S, 1000 * b + n, oracle if n <= 1 << 10 else None, host)
        assert redone == 0, (name, n, b, S, "the tail ran twice on uniform scalars")
    ctx.close()


@pytest.mark.parametrize("name", ["bls12_377", "pallas", "vesta"])
def test_short_parity_other_curves(oracle, libs, name):
    import sppark_amd
    fb = sppark_amd.msm.FP_BYTES[name]
    n = (1 << 10) + 3
    host = np.zeros((n, 2 * fb + 8), dtype=np.uint8)
    sppark_amd.generate_points(host, n, 77, 2 * fb + 8, name)
    import torch
    dev = torch.from_numpy(host).cuda()
    ctx = sppark_amd.MsmContext(name)
    for b, S in ((64, 8), (NBITS[name] - 2, 32)):
        assert check_cell(ctx, name, dev, n, b, S, 5 + b, oracle, host) == 0
    ctx.close()


@pytest.mark.parametrize("S", [16, 32])
def test_short_values_in_wider_slots(oracle, libs, S):
    """b = 64 at a stride of 16 and of 32 bytes, every byte above bit 64 random: the result is the MSM of the masked values"""
    import sppark_amd
    host, dev = points_of("bls12_381", 48)
    ctx = sppark_amd.MsmContext("bls12_381")
    for n in ((1 << 10) + 3, (1 << 14) + 7):
        check_cell(ctx, "bls12_381", dev, n, 64, S, 31 * S + n, oracle if n <= 1 << 10 else None, host)
    ctx.close()


def test_short_joined_path_2p22(libs):
    """2^22 points, b = 64: windows wide enough for k_join_runs (n / buckets <= 4 x run length); scalars made on the device"""
    import torch
    import sppark_amd
    n = 1 << 22
    pts = torch.zeros((n, 96), dtype=torch.uint8, device="cuda")
    sppark_amd.generate_progression(pts, n, 0x1234567, 0x9e3779b97f4a7c15, 96)
    sc = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device="cuda")
    wide = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    wide[:, 0] = sc
    ctx = sppark_amd.MsmContext("bls12_381")
    p, full = ctx.plan(n, scalar_bits=64), ctx.plan(n)
    assert n // p["buckets_per_window"] <= 4 * p["run_length"] and p["windows"] < full["windows"], (p, full)
    got = ctx.invoke(pts, sc, npoints=n, ffi_affine_sz=96, scalar_bits=64, scalar_stride=8)
    want = ctx.invoke(pts, wide, npoints=n, ffi_affine_sz=96)
    assert (affine(got, "bls12_381") == affine(want, "bls12_381")).all()
    assert (affine(got, "bls12_381") != 0).any()
    ctx.close()


@pytest.mark.parametrize("name", ["bls12_381", "bn254"])
def test_short_skewed_scalars(libs, name):
    """every scalar 2^b - 1 / 2^(b-1) (one bucket of the top window) / zero / one / every second one zero, handed over with
    every bit above b SET: equal to the yardstick (the piece tree may overflow here: the exact redo is allowed)"""
    import torch
    import sppark_amd
    fb = sppark_amd.msm.FP_BYTES[name]
    _, dev = points_of(name, fb)
    ctx = sppark_amd.MsmContext(name)
    for n in (255, (1 << 14) + 7):
        for b, S in ((8, 4), (33, 8), (64, 8), (65, 12), (129, 20)):
            rnd = int.from_bytes(random_slots(1, S, b).tobytes(), "little") % (1 << b)
            for what, values in (("2^b - 1", [(1 << b) - 1]), ("2^(b-1)", [1 << (b - 1)]), ("zero", [0]), ("one", [1]), ("half zero", [rnd, 0])):
                above = ((1 << (8 * S)) - 1) ^ ((1 << b) - 1)
                rows = [np.frombuffer((v | above).to_bytes(S, "little"), dtype=np.uint8) for v in values]
                raw = np.stack([rows[i % len(rows)] for i in range(n)])
                got = affine(ctx.invoke(dev[:n], torch.from_numpy(raw).cuda(), npoints=n, ffi_affine_sz=dev.shape[1],
                                        scalar_bits=b, scalar_stride=S), name)
                want = affine(ctx.invoke(dev[:n], torch.from_numpy(masked32(raw, b)).cuda(), npoints=n, ffi_affine_sz=dev.shape[1]), name)
                assert (got == want).all(), (name, n, b, S, what)
                if what == "zero":
                    assert (got == 0).all()
    ctx.close()


def test_short_plan_is_really_short(libs):
    import sppark_amd
    ctx = sppark_amd.MsmContext("bls12_381")
    n = 1 << 18
    full = ctx.plan(n)
    for b in (1, 8, 32, 64, 128, 253):
        p = ctx.plan(n, scalar_bits=b)
        assert p["windows"] == -(-(b + 1) // p["window_bits"]), (b, p)
        assert p["windows"] <= full["windows"]
    assert ctx.plan(n, scalar_bits=64)["windows"] < full["windows"]
    assert ctx.plan(1 << 26, scalar_bits=64)["windows"] == 3 and ctx.plan(1 << 26)["windows"] == 12
    ctx.close()


def test_short_other_paths(oracle, libs):
    """preloaded bases, a context with fixed-base tables (the short call takes the plain path over the points themselves),
    window groups, the chunked host path, host / device pointers mixed, reserve before invoke"""
    import torch
    import sppark_amd
    name = "bls12_381"
    host, dev = points_of(name, 48)
    n, b, S = (1 << 14) + 7, 64, 8
    raw = random_slots(n, S, 4711)
    wide = masked32(raw, b)
    d_raw = torch.from_numpy(raw).cuda()
    plain = sppark_amd.MsmContext(name)
    want = affine(plain.invoke(dev[:n], torch.from_numpy(wide).cuda(), npoints=n, ffi_affine_sz=104), name)
    assert (want != 0).any()

    def short(ctx, pts, sc, **kw):
        return affine(ctx.invoke(pts, sc, npoints=n, ffi_affine_sz=104, scalar_bits=b, scalar_stride=S, **kw), name)

    # reserve first: the invoke that follows allocates nothing
    ctx = sppark_amd.MsmContext(name)
    ctx.reserve(n, 104, scalar_bits=b, scalar_stride=S)
    held = ctx.scratch_bytes()
    assert held > 0
    assert (short(ctx, dev[:n], d_raw) == want).all() and ctx.scratch_bytes() == held
    # host / device pointers mixed (one chunk at this size)
    assert (short(ctx, host[:n], d_raw) == want).all(), "host points, device scalars"
    assert (short(ctx, dev[:n], raw) == want).all(), "device points, host scalars"
    assert (short(ctx, host[:n], raw) == want).all(), "host points, host scalars"
    # window groups
    ctx.tune_pipeline(groups=3)
    assert ctx.plan_groups(n) == 3
    assert (short(ctx, dev[:n], d_raw) == want).all(), "three window groups"
    b2 = 129
    raw2 = random_slots(n, 20, 4712)
    got2 = affine(ctx.invoke(dev[:n], torch.from_numpy(raw2).cuda(), npoints=n, ffi_affine_sz=104, scalar_bits=b2, scalar_stride=20), name)
    ctx.tune_pipeline()
    want2 = affine(ctx.invoke(dev[:n], torch.from_numpy(masked32(raw2, b2)).cuda(), npoints=n, ffi_affine_sz=104), name)
    assert (got2 == want2).all(), "three window groups, 129 bits"
    # the chunked host path: >= 3 chunks
    ctx.tune_pipeline(chunk_points=6000)
    assert (short(ctx, host[:n], raw) == want).all() and ctx.last_chunks() >= 3, "host buffers in chunks"
    assert (short(ctx, dev[:n], raw) == want).all() and ctx.last_chunks() >= 3, "host scalars in chunks"
    assert (short(ctx, dev[:n], d_raw) == want).all() and ctx.last_chunks() >= 3, "device buffers in chunks"
    ctx.tune_pipeline()
    # preloaded bases
    ctx.set_points(host[:n], ffi_affine_sz=104)
    assert (affine(ctx.invoke(None, d_raw, scalar_bits=b), name) == want).all(), "preloaded, device scalars"
    assert (affine(ctx.invoke(None, raw, scalar_bits=b), name) == want).all(), "preloaded, host scalars"
    m = 5000                                                    # a prefix of the preloaded set
    want_m = affine(plain.invoke(dev[:m], torch.from_numpy(wide[:m].copy()).cuda(), npoints=m, ffi_affine_sz=104), name)
    assert (affine(ctx.invoke(None, raw[:m].copy(), scalar_bits=b), name) == want_m).all(), "preloaded prefix"
    # fixed-base tables on the context: the short call falls back to the plain path over the points themselves
    ctx.tune(wbits=13)
    ctx.set_points(host[:n], ffi_affine_sz=104, fixed_base=True)
    ctx.tune(wbits=0)
    assert ctx.fixed_base_windows() > 0
    assert (affine(ctx.invoke(None, d_raw, scalar_bits=b), name) == want).all(), "fixed-base context, short call"
    assert (affine(ctx.invoke(None, torch.from_numpy(wide).cuda()), name) == want).all(), "fixed-base context, full-width call"
    ctx.close(); plain.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["wave_pairs", "one_lane"])
def test_short_g2_one_shot(oracle, libs, mode):
    """mult_pippenger_fp2_inf_bits at 2^12 points under both accumulation kernels: the same point as the full-width call"""
    import recipe
    import sppark_amd
    n, b, S = 1 << 12, 64, 8
    pts, _ = recipe.msm_inputs(2, n, 4242, ndistinct=512, flagged=True)
    raw = random_slots(n, S, 99)
    try:
        sppark_amd.set_g2_path(mode, "bls12_381")
        got = sppark_amd.multi_scalar_mult_fp2_arkworks(pts, raw, "bls12_381", scalar_bits=b)
        want = sppark_amd.multi_scalar_mult_fp2_arkworks(pts, masked32(raw, b), "bls12_381")
    finally:
        sppark_amd.set_g2_path(0, "bls12_381")
    assert (sppark_amd.to_affine_g2(got, "bls12_381") == sppark_amd.to_affine_g2(want, "bls12_381")).all()
    assert (sppark_amd.to_affine_g2(got, "bls12_381") != 0).any()
    # G1 one-shot
    host, _ = points_of("bls12_381", 48)
    got1 = sppark_amd.multi_scalar_mult_arkworks(host[:n], raw, "bls12_381", scalar_bits=b)
    want1 = sppark_amd.multi_scalar_mult_arkworks(host[:n], masked32(raw, b), "bls12_381")
    assert (affine(got1, "bls12_381") == affine(want1, "bls12_381")).all()


def test_short_refusals(libs):
    """outside the contract: a negative code with an owned message, out = infinity, and a correct next call on the same context
    (through the C ABI itself: the Python layer refuses the same arguments before it gets there)"""
    import torch
    import sppark_amd
    from sppark_amd import ffi
    name = "bls12_381"
    _, dev = points_of(name, 48)
    n = 255
    ctx = sppark_amd.MsmContext(name)
    L = ctx.L
    buf = torch.from_numpy(random_slots(n + 1, 32, 5)).cuda()
    base = buf.data_ptr()
    assert base % 16 == 0
    for what, bits, S, ptr in (("b = 0", 0, 4, base), ("b = NBITS - 1", NBITS[name] - 1, 32, base), ("S = 4 with b = 33", 33, 4, base),
                               ("S = 6", 8, 6, base), ("S = 36", 64, 36, base), ("misaligned for S = 8", 64, 8, base + 4)):
        out = np.full(144, 0xff, dtype=np.uint8)
        err = L.sppark_msm_invoke_bits(ctx.h, out.ctypes.data, dev.data_ptr(), n, ptr, bits, S, 104)
        assert err.code < 0 and err.message, what
        msg = ctypes.string_at(err.message).decode()
        L.drop_error_message(err.message)
        assert "invalid argument" in msg, (what, msg)
        assert (out == 0).all(), what
        out = np.full(144, 0xff, dtype=np.uint8)
        err = L.mult_pippenger_inf_bits(out.ctypes.data, dev.data_ptr(), n, ptr, bits, S, 104)
        assert err.code < 0 and err.message and (out == 0).all(), what
        L.drop_error_message(err.message)
        err = L.sppark_msm_reserve_bits(ctx.h, n, 104, 0, 0, bits, S)
        if what != "misaligned for S = 8":
            assert err.code < 0 and err.message, what
            L.drop_error_message(err.message)
        with pytest.raises(ValueError):
            ctx.invoke(dev[:n], ptr, npoints=n, ffi_affine_sz=104, scalar_bits=bits, scalar_stride=S)
        # the context is as it was: a correct call
        check_cell(ctx, name, dev, n, 64, 8, 17)
    with pytest.raises(ffi.SpparkError):                        # more scalars than preloaded points: the ordinary refusals still hold
        ctx.invoke(None, buf[:n].contiguous(), scalar_bits=64, scalar_stride=32)
    ctx.close()
