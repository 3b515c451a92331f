"""GPU: sppark_ntt_batch / sppark_lde_batch (include/sppark_amd_batch.h) through the C ABI.

Every column of a batched call is held against sppark_ntt / sppark_lde on that column alone (the single-transform path, itself
held against the oracle by the other NTT tests), in all nine NTT libraries and all 16 modes, at every size of the packed
kernel (2^1 ... 2^6, several columns per wave), of k_ntt_small, and at the plan boundaries above; sampled columns also
against the oracle directly.  Then the layouts (gaps between columns that stay untouched, torch row views, numpy host
buffers, host chunks), the streams, launch chunks above the grid limit, a batch past 2^32 elements, and every rejected
argument."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NARROW = ["gl64", "bb31", "gl64_plonky2", "bb31_canonical"]
WIDE = ["bls12_381", "bn254", "bls12_377", "pallas", "vesta"]
LIBS = NARROW + WIDE
CHUNK = 256 << 20                                                   # SPPARK_BATCH_CHUNK_BYTES
# every size of the packed kernel and of k_ntt_small, and the plan boundaries above them (narrow: the radix-64 plan from
# 2^12, a generic top pass 2^13, k_ntt6 on top at 2^18, one inter-pass table up to 2^20; wide: k_ntt_pass_lat from 2^10)
LGS = {"narrow": list(range(1, 14)) + [16, 18, 20], "wide": list(range(1, 11)) + [12, 16]}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _eb(field):
    return 32 if field in WIDE else 8 if field.startswith("gl64") else 4


def _p(field):
    return (1 << 64) - (1 << 32) + 1 if field.startswith("gl64") else 2013265921


def _rand(field, rows, n, seed, device="cuda"):
    """rows x n field elements (wide fields: n x 4 u64 words per row, top limb masked below r) as a torch tensor"""
    torch = _torch()
    g = torch.Generator(device=device).manual_seed(seed)
    if field in WIDE:
        x = torch.randint(-(1 << 63), (1 << 63) - 1, (rows, n, 4), dtype=torch.int64, device=device, generator=g)
        x[:, :, 3] &= (1 << 60) - 1                                 # < 2^252 < r for every curve here
        return x.reshape(rows, 4 * n)
    if field.startswith("gl64"):
        x = torch.randint(-(1 << 63), (1 << 63) - 1, (rows, n), dtype=torch.int64, device=device, generator=g)
        return torch.where((x < 0) & (x > -(1 << 32)), x + (1 << 32), x)          # (u64 values >= p folded below 2^32)
    return torch.randint(0, _p(field), (rows, n), dtype=torch.int32, device=device, generator=g)


def _lib(field):
    from sppark_amd import ffi
    return ffi.load(field)


def _check(L, err):
    from sppark_amd import ffi
    ffi.check(L, err)


def _single_cols(L, x, lg, order, direction, typ, stream):
    """sppark_ntt on every row of |x| (in place), on |stream|"""
    for j in range(x.shape[0]):
        _check(L, L.sppark_ntt(0, x[j].data_ptr(), lg, order, direction, typ, stream))


@pytest.fixture(scope="module")
def stream():
    torch = _torch()
    return torch.cuda.Stream()


@pytest.mark.parametrize("field", LIBS)
def test_every_column_equals_sppark_ntt(libs, field, stream):
    torch = _torch()
    L = _lib(field)
    h = stream.cuda_stream
    for lg in LGS["wide" if field in WIDE else "narrow"]:
        n = 1 << lg
        big = 300 if lg <= 6 else 37                                # (300 at 2^1: a full work-group of 256 columns and a partial one)
        x = _rand(field, big, n, 1000 + lg)
        for mode in range(16):
            order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
            ref = x.clone()
            torch.cuda.synchronize()
            _single_cols(L, ref, lg, order, direction, typ, h)
            outs = []
            for b in (1, 3, 37, 300) if big == 300 else (1, 3, 37):
                y = x[:b].clone()
                torch.cuda.synchronize()
                _check(L, L.sppark_ntt_batch(0, y.data_ptr(), lg, b, 0, order, direction, typ, h))
                outs.append(y)
            stream.synchronize()
            for y in outs:
                assert torch.equal(y, ref[:y.shape[0]]), (field, lg, mode, y.shape[0])


@pytest.mark.parametrize("field", ["gl64", "bb31", "bls12_381"])
def test_sampled_columns_against_the_oracle(libs, oracle, field):
    torch = _torch()
    import sppark_amd
    O = oracle
    if field in WIDE:
        f = lambda a, o, d, t: O.ntt_fr(O.CURVE_ID[field], a, o, d, t)
    else:
        f = O.ntt_gl64 if field == "gl64" else O.ntt_bb31
    for lg, b in ((2, 300), (6, 40), (9, 5), (12, 3)) if field in WIDE else ((2, 300), (6, 40), (9, 5), (13, 3), (16, 3)):
        x = _rand(field, b, 1 << lg, 7 * lg)
        xh = x.cpu().numpy()
        for mode in (0, 1, 6, 7, 9, 14, 15):
            order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
            y = x.clone()
            sppark_amd.compute_ntt_batch(0, y, order, direction, typ, field)
            yh = y.cpu().numpy()
            for j in sorted({0, b // 2, b - 1}):
                col = xh[j].view(np.uint64).reshape(-1, 4) if field in WIDE else xh[j].view(np.uint64 if field == "gl64" else np.uint32)
                exp = f(col.copy(), order, direction, typ)
                got = yh[j].view(np.uint64).reshape(-1, 4) if field in WIDE else yh[j].view(exp.dtype)
                assert (got == exp).all(), (field, lg, mode, j)


@pytest.mark.parametrize("field", ["gl64", "bb31", "bls12_381"])
def test_layouts_gaps_views_and_host_buffers(libs, field):
    torch = _torch()
    import sppark_amd
    L = _lib(field)
    w = 4 if field in WIDE else 1                                   # tensor words per element
    for lg in (1, 5, 8, 11, 12, 14):
        n = 1 << lg
        # gaps: odd below 2^12; whole 16-byte units from 2^12 on (where k_ntt12 moves 16 bytes per access)
        gap = 3 if lg < 12 or field in WIDE else 16 // _eb(field)
        b = 21
        x = _rand(field, b, n, 300 + lg)
        sentinel = 0x5A5A5A5A
        buf = torch.full((b, (n + gap) * w), sentinel, dtype=x.dtype, device="cuda")
        buf[:, :n * w] = x
        for mode in (1, 6, 11, 12):
            order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
            ref = x.clone()
            _single_cols(L, ref, lg, order, direction, typ, None)
            y = buf.clone()
            sppark_amd.compute_ntt_batch(0, y[:, :n * w], order, direction, typ, field)      # a torch row view: stride n + gap
            assert torch.equal(y[:, :n * w], ref), (field, lg, mode)
            assert bool((y[:, n * w:] == sentinel).all()), "gap written"
            yh = buf.cpu().numpy()                                  # the same on a numpy host buffer (2-D copies, no gaps moved)
            sppark_amd.compute_ntt_batch(0, yh[:, :n * w], order, direction, typ, field)
            assert (yh[:, :n * w] == ref.cpu().numpy()).all() and (yh[:, n * w:] == sentinel).all(), (field, lg, mode)


@pytest.mark.parametrize("field", ["gl64", "bb31"])
def test_columns_off_16_byte_alignment(libs, field):
    """stride 2^lg + 1 from 2^12 on: every other column starts off a 16-byte boundary where k_ntt12 moves 16 bytes per access
    (as sppark_ntt on a view at an odd element offset)"""
    torch = _torch()
    L = _lib(field)
    for lg in (12, 13, 16):
        n, b = 1 << lg, 7
        x = _rand(field, b, n, 500 + lg)
        sentinel = 0x5A5A5A5A
        buf = torch.full((b, n + 1), sentinel, dtype=x.dtype, device="cuda")
        buf[:, :n] = x
        for mode in range(16):
            order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
            ref = x.clone()
            _single_cols(L, ref, lg, order, direction, typ, None)
            y = buf.clone()
            _check(L, L.sppark_ntt_batch(0, y.data_ptr(), lg, b, n + 1, order, direction, typ, None))
            assert torch.equal(y[:, :n], ref), (field, lg, mode)
            assert bool((y[:, n:] == sentinel).all()), "gap written"


def test_streams_enqueue_or_synchronise(libs):
    torch = _torch()
    L = _lib("gl64")
    x = _rand("gl64", 64, 1 << 12, 5)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(200_000_000)                              # keeps |s| busy well past the call's return
    _check(L, L.sppark_ntt_batch(0, x.data_ptr(), 12, 64, 0, 1, 0, 0, s.cuda_stream))
    assert not s.query(), "a non-NULL stream: the call only enqueues"
    s.synchronize()
    torch.cuda._sleep(200_000_000)                                  # the NULL stream (torch's default here)
    _check(L, L.sppark_ntt_batch(0, x.data_ptr(), 12, 64, 0, 2, 1, 0, None))
    assert torch.cuda.current_stream().query(), "the NULL stream: the call returns when the work is done"
    ref = _rand("gl64", 64, 1 << 12, 5)
    assert torch.equal(x, ref)                                      # forward NR then inverse RN


def test_host_batch_above_the_chunk(libs):
    """a numpy batch of 1100 Goldilocks columns of 2^16 (550 MB): chunks of 512 columns, the last one ragged"""
    torch = _torch()
    L = _lib("gl64")
    lg, b = 16, 1100
    assert b * (8 << lg) > 2 * CHUNK and (b * (8 << lg)) % CHUNK
    x = _rand("gl64", b, 1 << lg, 11)
    for mode in (1, 14):
        order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
        d = x.clone()
        _check(L, L.sppark_ntt_batch(0, d.data_ptr(), lg, b, 0, order, direction, typ, None))
        h = x.cpu().numpy()
        _check(L, L.sppark_ntt_batch(0, h.ctypes.data, lg, b, 0, order, direction, typ, None))
        assert (h == d.cpu().numpy()).all(), mode
        ref = x[[0, 511, 512, 1023, 1024, b - 1]].clone()
        _single_cols(L, ref, lg, order, direction, typ, None)
        assert (h[[0, 511, 512, 1023, 1024, b - 1]] == ref.cpu().numpy()).all(), mode


@pytest.mark.parametrize("lg", [2, 13])
def test_launch_chunks_above_the_grid_limit(libs, lg):
    torch = _torch()
    L = _lib("bb31")
    per = L.sppark_ntt_batch_launch_cols(0, lg)
    assert per > 0
    b = per + 3
    assert b * (4 << lg) <= (8 << 30), ("launch chunk of %d columns" % per)
    x = _rand("bb31", b, 1 << lg, 13 + lg)
    cols = sorted({0, 1, per // 2, per - 1, per, per + 1, b - 1})
    for mode in (1, 6, 15):
        order, direction, typ = mode >> 2, (mode >> 1) & 1, mode & 1
        y = x.clone()
        _check(L, L.sppark_ntt_batch(0, y.data_ptr(), lg, b, 0, order, direction, typ, None))
        ref = x[cols].clone()
        _single_cols(L, ref, lg, order, direction, typ, None)
        assert torch.equal(y[cols], ref), (lg, mode)
        del y


def test_batch_past_2_to_the_32_elements(libs):
    """BabyBear 2^12 x (2^20 + 1) columns on the device: 2^32 + 2^12 elements, 16 GB"""
    torch = _torch()
    L = _lib("bb31")
    lg, b = 12, (1 << 20) + 1
    x = _rand("bb31", b, 1 << lg, 17)
    rng = np.random.default_rng(3)
    cols = sorted({0, 1, (1 << 19) + 7, (1 << 20) - 1, 1 << 20} | set(int(v) for v in rng.integers(0, b, 16)))
    keep = x[cols].clone()
    _check(L, L.sppark_ntt_batch(0, x.data_ptr(), lg, b, 0, 1, 0, 1, None))           # forward coset NR
    _single_cols(L, keep, lg, 1, 0, 1, None)
    assert torch.equal(x[cols], keep)
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lgd,lgb", [(1, 1), (0, 2)])
def test_lde_batch_above_the_grid_limit(libs, lgd, lgb):
    """more LDE columns than the grid's y dimension at extended sizes of the packed kernel: the spread before it (a grid row
    per column) runs in several launches"""
    torch = _torch()
    L = _lib("bb31")
    rows = L.sppark_ntt_batch_launch_cols(0, 13)                    # (2^13: one grid row per column -- the grid's y limit)
    assert rows > 0 and L.sppark_ntt_batch_launch_cols(0, lgd + lgb) > rows
    dom, ext, b = 1 << lgd, 1 << (lgd + lgb), rows + 3
    x = _rand("bb31", b, ext, 61 + lgd)
    y, aux = x.clone(), torch.zeros((b, dom), dtype=torch.int32, device="cuda")
    _check(L, L.sppark_lde_batch(0, y.data_ptr(), lgd, lgb, b, aux.data_ptr(), None))
    cols = sorted({0, 1, rows - 1, rows, rows + 1, b - 1})
    ref, ref_aux = x[cols].clone(), torch.zeros((len(cols), dom), dtype=torch.int32, device="cuda")
    for j in range(len(cols)):
        _check(L, L.sppark_lde(0, ref[j].data_ptr(), lgd, lgb, ref_aux[j].data_ptr(), None))
    assert torch.equal(y[cols], ref) and torch.equal(aux[cols], ref_aux)


LDE_CASES = {"narrow": [(0, 0), (0, 2), (3, 2), (5, 1), (9, 3), (10, 2), (11, 1), (13, 3), (8, 4), (7, 5)],
             "wide": [(0, 0), (0, 2), (3, 2), (5, 1), (8, 3), (7, 4), (10, 2)]}


@pytest.mark.parametrize("field", LIBS)
def test_lde_batch_equals_sppark_lde(libs, field):
    torch = _torch()
    L = _lib(field)
    w = 4 if field in WIDE else 1
    for lgd, lgb in LDE_CASES["wide" if field in WIDE else "narrow"]:
        dom, ext, b = 1 << lgd, 1 << (lgd + lgb), 5
        x = _rand(field, b, ext, 40 + lgd * 8 + lgb)
        ref, ref_aux = x.clone(), torch.zeros((b, dom * w), dtype=x.dtype, device="cuda")
        for j in range(b):
            _check(L, L.sppark_lde(0, ref[j].data_ptr(), lgd, lgb, ref_aux[j].data_ptr(), None))
        y, aux = x.clone(), torch.zeros_like(ref_aux)
        _check(L, L.sppark_lde_batch(0, y.data_ptr(), lgd, lgb, b, aux.data_ptr(), None))
        assert torch.equal(y, ref) and torch.equal(aux, ref_aux), (field, lgd, lgb)
        yh, auxh = x.cpu().numpy(), np.zeros((b, dom * w), dtype=ref_aux.cpu().numpy().dtype)
        _check(L, L.sppark_lde_batch(0, yh.ctypes.data, lgd, lgb, b, auxh.ctypes.data, None))
        assert (yh == ref.cpu().numpy()).all() and (auxh == ref_aux.cpu().numpy()).all(), (field, lgd, lgb, "host")
        y = x.clone()                                               # without the coefficients
        _check(L, L.sppark_lde_batch(0, y.data_ptr(), lgd, lgb, b, None, None))
        assert torch.equal(y, ref), (field, lgd, lgb, "no aux")


def test_lde_host_chunks_and_scratch_bound(libs):
    """700 host columns of 2^14 -> 2^16 with host coefficients: 768 KB of device scratch per column, 341 columns per chunk"""
    torch = _torch()
    L = _lib("gl64")
    lgd, lgb, b = 14, 2, 700
    dom, ext = 1 << lgd, 1 << (lgd + lgb)
    x = _rand("gl64", b, ext, 91)
    d, d_aux = x.clone(), torch.zeros((b, dom), dtype=torch.int64, device="cuda")
    _check(L, L.sppark_lde_batch(0, d.data_ptr(), lgd, lgb, b, d_aux.data_ptr(), None))
    L.sppark_ntt_release_cached()
    h, h_aux = x.cpu().numpy(), np.zeros((b, dom), dtype=np.int64)
    _check(L, L.sppark_lde_batch(0, h.ctypes.data, lgd, lgb, b, h_aux.ctypes.data, None))
    assert (h == d.cpu().numpy()).all() and (h_aux == d_aux.cpu().numpy()).all()
    col_need = (2 * dom + ext) * 8
    assert L.sppark_ntt_cached_scratch_bytes() <= max(col_need, CHUNK)
    L.sppark_ntt_release_cached()                                   # one column above the chunk: one column of scratch
    lgd, lgb, b = 21, 4, 2                                          # (2^21 -> 2^25: 320 MB per column)
    col_need = ((1 << lgd) + (1 << (lgd + lgb))) * 8
    assert col_need > CHUNK
    xh = np.zeros((b, 1 << (lgd + lgb)), dtype=np.uint64)
    xh[:, :1 << lgd] = _rand("gl64", b, 1 << lgd, 92).cpu().numpy().view(np.uint64)
    ref = torch.from_numpy(xh.view(np.int64).copy()).cuda()
    for j in range(b):
        _check(L, L.sppark_lde(0, ref[j].data_ptr(), lgd, lgb, None, None))
    L.sppark_ntt_release_cached()
    _check(L, L.sppark_lde_batch(0, xh.ctypes.data, lgd, lgb, b, None, None))
    assert L.sppark_ntt_cached_scratch_bytes() <= max(col_need, CHUNK)
    assert (xh.view(np.int64) == ref.cpu().numpy()).all()


@pytest.mark.parametrize("field", ["gl64", "bls12_381"])
def test_rejected_arguments_leave_the_buffer_alone(libs, field):
    torch = _torch()
    L = _lib(field)
    lg, b = 6, 3
    n = 1 << lg
    x = _rand(field, b, n, 77)
    keep = x.clone()
    two_adic = 33                                                   # (Goldilocks and BLS12-381 Fr: 2-adicity 32)

    def rejected(err):
        assert err.code < 0 and err.message, field
        msg = ctypes.string_at(err.message)
        L.drop_error_message(err.message)
        assert torch.equal(x, keep), "buffer changed"
        return msg
    p = x.data_ptr()
    rejected(L.sppark_ntt_batch(0, p, two_adic, b, 0, 1, 0, 0, None))
    rejected(L.sppark_ntt_batch(0, p, lg, b, 0, 4, 0, 0, None))
    rejected(L.sppark_ntt_batch(0, p, lg, b, 0, -1, 0, 0, None))
    assert b"stride" in rejected(L.sppark_ntt_batch(0, p, lg, b, n - 1, 1, 0, 0, None))
    rejected(L.sppark_ntt_batch(0, p, lg, 1 << 62, 0, 1, 0, 0, None))                 # bytes overflow size_t
    rejected(L.sppark_ntt_batch(0, p, lg, 1 << 40, 1 << 20, 1, 0, 0, None))
    rejected(L.sppark_lde_batch(0, p, two_adic - 2, 3, 1, None, None))
    rejected(L.sppark_lde_batch(0, p, lg, 2, 1 << 60, None, None))                    # bytes overflow size_t
    assert L.sppark_ntt_batch(0, p, lg, 0, 0, 1, 0, 0, None).code == 0                # batch == 0: no-op
    assert L.sppark_lde_batch(0, p, lg, 1, 0, None, None).code == 0
    assert L.sppark_ntt_batch(0, p, 0, b, 0, 1, 0, 0, None).code == 0                 # lg == 0: no-op
    assert torch.equal(x, keep)
    # extents past the end of an allocation of exactly 4 columns (hipMalloc through the library: no allocator slack
    # behind it); the buffer is filled and read back through sppark_lde_expand (blow-up 1 = a copy)
    L.sppark_gpu_ptr_alloc.argtypes = [ctypes.c_size_t]; L.sppark_gpu_ptr_alloc.restype = ctypes.c_void_p
    L.sppark_gpu_ptr_get.argtypes = [ctypes.POINTER(ctypes.c_void_p)]; L.sppark_gpu_ptr_get.restype = ctypes.c_void_p
    ref = ctypes.c_void_p(L.sppark_gpu_ptr_alloc(4 * n * _eb(field)))
    raw = L.sppark_gpu_ptr_get(ctypes.byref(ref))
    try:
        src = _rand(field, 4, n, 78)
        _check(L, L.sppark_lde_expand(0, raw, src.data_ptr(), lg + 2, 0, None))
        assert b"past" in rejected(L.sppark_ntt_batch(0, raw, lg, 5, 0, 1, 0, 0, None))
        assert b"past" in rejected(L.sppark_ntt_batch(0, raw, lg, 2, 3 * n + 1, 1, 0, 0, None))
        assert b"past" in rejected(L.sppark_lde_batch(0, raw, lg, 1, 3, None, None))
        assert b"past" in rejected(L.sppark_lde_batch(0, x.data_ptr(), lg - 2, 0, 2, raw + (4 * n - 8) * _eb(field), None))
        back = torch.zeros_like(src)
        _check(L, L.sppark_lde_expand(0, back.data_ptr(), raw, lg + 2, 0, None))
        assert torch.equal(back, src), "rejected call changed the allocation"
        _check(L, L.sppark_ntt_batch(0, raw, lg, 4, 0, 1, 0, 0, None))                 # the whole allocation: accepted
    finally:
        L.drop_gpu_ptr_t(ctypes.byref(ref))
