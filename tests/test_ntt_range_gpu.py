"""GPU: the NTT over the whole size range the entry points accept, beyond 2^24.

Above 2^24 the plans change shape (ntt_r64_kernels.hpp make_r64_plan: [7, 6] ... [8, 8] above k_ntt12 at lg 25 ... 28, a
generic pass below the top at 27 and 28, so the coset runs as k_coset there; [5, 6, 6] ... [8, 6, 6] at 29 ... 32), and the
256-bit passes generate their twiddles per element (ntt_driver.hpp wide_table_lg: tables up to 2^24 entries only).  A root
that forward and inverse share, or an index error the inverse undoes, passes every round trip, so each size is compared with
an exact result:

  (a) up to the reference's MAX_LG_DOMAIN_SIZE (28; BabyBear 27), the reference's own HIP build on the same device memory
      (oracle.ref_ntt_dev), whole outputs;
  (b) above it, the closed form of a periodic input (tests/golden/ntt_closed_form.py, pinned on the CPU by
      tests/test_ntt_closed_form.py) at every power-of-two boundary, the ends and 4096 random positions, and a dense random
      round trip;
  (c) sppark_lde at extended sizes 2^23 ... 2^28 against the reference's NTT::LDE_aux, the aux output included.

Inputs are made on the device (a 2^28 256-bit array is 8 GB).  Each leg skips, naming its size, when it needs more than half
the free device memory; every buffer is freed before the next leg."""
import gc

import numpy as np
import pytest

import ntt_closed_form as C

pytestmark = pytest.mark.gpu
NN, NR, RN, RR = 0, 1, 2, 3
WIDE = list(C.WIDE)
ALL16 = C.MODES
FEW = [(NR, 0, 0), (RN, 1, 0), (NN, 0, 0), (NN, 0, 1), (NN, 1, 1)]
KIND = {"gl64_plonky2": "gl64", "bb31_canonical": "bb31"}
TWO_ADICITY = {"gl64": 32, "bb31": 27, "bls12_381": 32, "bn254": 28, "bls12_377": 47, "pallas": 32, "vesta": 32}
CHUNK = 1 << 25
THREADS = 16


def _w(kind):
    return 4 if kind in WIDE else 1


def _tdt(kind):
    import torch
    return torch.int32 if kind == "bb31" else torch.int64


def _elem_bytes(kind):
    return 32 if kind in WIDE else (4 if kind == "bb31" else 8)


def _signed(v, kind):
    """limbs of the raw word |v| as the signed values of the device tensor"""
    bits = 32 if kind == "bb31" else 64
    out = []
    for k in range(_w(kind)):
        x = (v >> (bits * k)) & ((1 << bits) - 1)
        out.append(x - (1 << bits) if x >> (bits - 1) else x)
    return out


def _modulus(O, kind):
    return O.FR_MODULUS[O.CURVE_ID[kind]] if kind in WIDE else (O.GL64_P if kind == "gl64" else O.BB31_P)


def _need_mem(nbytes):
    import torch
    free, _ = torch.cuda.mem_get_info()
    if nbytes > free // 2:
        pytest.skip("needs %.1f GB of device memory, half the free memory is %.1f GB" % (nbytes / 2**30, free / 2**31))


def _release(*libs):
    import torch
    from sppark_amd import ffi
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    for lib in libs:
        ffi.load(lib).sppark_ntt_release_cached()


def _rand_chunk(O, kind, m, gen):
    """m uniform raw words below the modulus (256-bit: top limb below the modulus's top limb), flat"""
    import torch
    dev = "cuda"
    if kind == "bb31":
        return torch.randint(0, O.BB31_P, (m,), generator=gen, device=dev, dtype=torch.int32)

    def u64(k):
        hi = torch.randint(-(1 << 31), 1 << 31, (k,), generator=gen, device=dev, dtype=torch.int64)
        lo = torch.randint(0, 1 << 32, (k,), generator=gen, device=dev, dtype=torch.int64)
        return (hi << 32) | lo
    if kind == "gl64":
        r = u64(m)                                            # [p, 2^64) as signed: [-(2^32 - 1), -1]; subtract p
        return torch.where((r < 0) & (r >= -((1 << 32) - 1)), r + ((1 << 32) - 1), r)
    r = u64(4 * m).view(m, 4)
    r[:, 3] = torch.randint(0, _modulus(O, kind) >> 192, (m,), generator=gen, device=dev, dtype=torch.int64)
    return r.reshape(-1)


def _rand_fill(O, kind, buf, seed):
    """uniform raw words with 0, 1, p - 1 in front; chunk c comes from its own generator (seed, c): refillable"""
    import torch
    w = _w(kind)
    n = buf.numel() // w
    for c0 in range(0, n, CHUNK):
        m = min(CHUNK, n - c0)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(seed * 100003 + c0 // CHUNK)
        buf[c0 * w:(c0 + m) * w] = _rand_chunk(O, kind, m, gen)
    p = _modulus(O, kind)
    for i, v in enumerate((0, 1, p - 1)[:n]):
        buf[i * w:(i + 1) * w] = torch.tensor(_signed(v, kind), dtype=buf.dtype, device="cuda")
    return buf


def _bitrev_dev(i, lg, tab):
    r = (tab[i & 0xffff] << 16) | tab[(i >> 16) & 0xffff]
    return r >> (32 - lg)


def _periodic_fill(buf, T, lg, rev, tab):
    """buf[i] = T[i mod K] (rev: position i holds T[rev(i) mod K])"""
    import torch
    K, w = T.shape
    n = 1 << lg
    v = buf.view(n, w)
    for c0 in range(0, n, CHUNK):
        i = torch.arange(c0, min(n, c0 + CHUNK), device="cuda", dtype=torch.int64)
        if rev:
            i = _bitrev_dev(i, lg, tab)
        v[c0:c0 + i.numel()] = T[i % K]


def _gather(buf, kind, lg, pos):
    import torch
    w = _w(kind)
    rows = buf.view(1 << lg, w)[torch.from_numpy(pos).cuda()].cpu().numpy()
    return rows.view(np.uint32 if kind == "bb31" else np.uint64).reshape(-1, w) if w > 1 else rows.view(
        np.uint32 if kind == "bb31" else np.uint64).reshape(-1)


# ------------------------------------------------------------------ (a) the reference build, on device memory ----
def _need_ref(O, lib):
    if not O.ref_ntt_available(lib):
        pytest.skip("oracle/_ref/libref_ntt_%s.so is not built (oracle/Makefile ref_ntt needs /root/reference at BUILD time)" % lib)


def _ref_cases():
    cases = [("gl64", lg, ALL16) for lg in range(24, 29)] + [("bb31", lg, ALL16) for lg in range(24, 28)]
    for f in WIDE:
        cases += [(f, lg, ALL16 if lg in (23, 24, 25, 28) else FEW) for lg in range(21, 29)]
    cases += [("gl64_plonky2", 28, [(NR, 0, 0), (RN, 1, 0)]), ("bb31_canonical", 27, [(NR, 0, 0), (RN, 1, 0)])]
    return cases


@pytest.mark.parametrize("lib,lg,modes", _ref_cases(), ids=lambda v: "" if isinstance(v, list) else str(v))
def test_ntt_large_sizes_equal_the_reference_build(oracle, libs, lib, lg, modes):
    """compute_ntt and the reference's NTT::Base_dev_ptr on two copies of the same device array, whole outputs"""
    import torch
    import sppark_amd
    O = oracle
    _need_ref(O, lib)
    kind = KIND.get(lib, lib)
    n, w = 1 << lg, _w(kind)
    _need_mem(2 * n * _elem_bytes(kind))
    a = torch.empty(n * w, dtype=_tdt(kind), device="cuda")
    b = torch.empty_like(a)
    try:
        for order, direction, typ in modes:
            _rand_fill(O, kind, a, 7 * lg + 2 * order + direction)
            b.copy_(a)
            torch.cuda.synchronize()
            sppark_amd.compute_ntt(0, a, order, direction, typ, lib)
            O.ref_ntt_dev(lib, b.data_ptr(), lg, order, direction, typ)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (lib, lg, order, direction, typ)
    finally:
        del a, b
        _release(lib)


# ------------------------------------------------------- (b) closed form above the reference's range ----
CLOSED = [("gl64", lg) for lg in range(29, 33)] + [("bls12_381", 29), ("bls12_381", 30)]


@pytest.mark.parametrize("field,lg", CLOSED)
def test_ntt_above_the_reference_range_closed_form(oracle, libs, field, lg):
    """all 16 modes on a periodic input of prime period K (65521; 256-bit: 4093) at ~5000 positions against the closed form
    (forward coset RR, whose factors g^rev(i) break the period: a sparse input's exact output instead), then dense random
    NR -> RN and coset RR forward -> inverse round trips compared with the regenerated input on the device"""
    import torch
    import sppark_amd
    O = oracle
    F = C.Field(O, field)
    n, w = 1 << lg, _w(field)
    _need_mem(n * _elem_bytes(field) + (256 << 20))
    K = 4093 if field in WIDE else 65521
    rng = np.random.default_rng(lg)
    t = [0, 1, F.p - 1] + [int.from_bytes(rng.bytes(40), "little") % F.p for _ in range(K - 3)]
    T_host = F.from_ints(t).reshape(K, w)
    pc = C.Periodic(F, lg, T_host)
    pos = C.positions(lg, 4096, 100 + lg)
    sp_pos = np.unique(np.concatenate([[0, 1, n - 1, 1 << 12, (1 << 18) + 1, (1 << 24) - 1, n >> 1],
                                       rng.integers(0, n, size=9)]))
    sp = C.Sparse(F, lg, sp_pos, F.from_ints(t[3:3 + len(sp_pos)]))
    cache = {}

    def expected(order, direction, typ):
        if order == RR and direction == 0 and typ == 1:
            return sp.values(order, direction, typ, pos)
        key = (order == NR, direction, typ, order == RR and direction == 1 and typ == 1)
        if key not in cache:
            cache[key] = pc.values(order, direction, typ, pos, threads=THREADS)
        return cache[key]

    tab = torch.from_numpy(C.bitrev(np.arange(1 << 16), 16)).cuda()
    T = torch.from_numpy(T_host.view(np.int64)).cuda()
    buf = torch.empty(n * w, dtype=torch.int64, device="cuda")
    try:
        for order, direction, typ in ALL16:
            if order == RR and direction == 0 and typ == 1:
                buf.zero_()
                buf.view(n, w)[torch.from_numpy(sp_pos).cuda()] = torch.from_numpy(
                    F.from_ints(sp.vals).reshape(-1, w).view(np.int64)).cuda()
            else:
                _periodic_fill(buf, T, lg, order == RN, tab)
            torch.cuda.synchronize()
            sppark_amd.compute_ntt(0, buf, order, direction, typ, field)
            got = _gather(buf, field, lg, pos)
            bad = C.mismatches(F, expected(order, direction, typ), got)
            assert not bad, (field, lg, order, direction, typ, len(bad), pos[bad[:8]].tolist())
        for fwd, inv, typ in ((NR, RN, 0), (RR, RR, 1)):
            _rand_fill(O, field, buf, 11 * lg + typ)
            sppark_amd.compute_ntt(0, buf, fwd, 0, typ, field)
            sppark_amd.compute_ntt(0, buf, inv, 1, typ, field)
            chk = torch.empty(CHUNK * w, dtype=torch.int64, device="cuda")
            for c0 in range(0, n, CHUNK):
                gen = torch.Generator(device="cuda")
                gen.manual_seed((11 * lg + typ) * 100003 + c0 // CHUNK)
                chk.copy_(_rand_chunk(O, field, CHUNK, gen))
                if c0 == 0:
                    for i, v in enumerate((0, 1, F.p - 1)):
                        chk[i * w:(i + 1) * w] = torch.tensor(_signed(v, field), dtype=torch.int64, device="cuda")
                assert torch.equal(buf[c0 * w:(c0 + CHUNK) * w], chk), (field, lg, "round trip", fwd, typ, c0)
            del chk
    finally:
        del buf, T, tab
        _release(field)


# ------------------------------------------------------------------------ (c) LDE at extended sizes ----
def _lde_cases():
    out = []
    for lib, top in (("gl64", 28), ("bb31", 27)):
        for ext in range(23, top + 1):
            out += [(lib, ext - b, b) for b in (1, 2, 3)]
        out += [(lib, 23 - 4, 4), (lib, top - 5, 5)]
    return out


@pytest.mark.parametrize("lib,lg,lgb", _lde_cases())
def test_lde_extended_sizes_equal_the_reference_build(oracle, libs, lib, lg, lgb):
    """sppark_lde on device tensors (blow-ups 1 ... 3: the spread fused into the first k_ntt12; 4, 5: the separate spread)
    against NTT::LDE_aux of the reference's build, evaluations and aux coefficients"""
    import torch
    import sppark_amd
    O = oracle
    _need_ref(O, lib)
    kind = KIND.get(lib, lib)
    dt, sdt = (np.uint32, np.int32) if kind == "bb31" else (np.uint64, np.int64)
    _need_mem(3 * (1 << (lg + lgb)) * _elem_bytes(kind))
    rng = np.random.default_rng(lg * 8 + lgb)
    p = _modulus(O, kind)
    x = (rng.integers(0, 1 << 63, size=1 << lg, dtype=np.uint64) % np.uint64(p)).astype(dt)
    x[:3] = np.array([0, 1, p - 1], dtype=dt)
    ref, ref_aux = O.ref_lde(lib, x, lgb, want_aux=True)
    d = torch.zeros(1 << (lg + lgb), dtype=_tdt(kind), device="cuda")
    d[:1 << lg] = torch.from_numpy(x.view(sdt)).cuda()
    aux = torch.zeros(1 << lg, dtype=_tdt(kind), device="cuda")
    try:
        sppark_amd.LDE(0, d, lg, lgb, lib, aux_out=aux, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(d, torch.from_numpy(ref.view(sdt)).cuda()), (lib, lg, lgb)
        assert torch.equal(aux, torch.from_numpy(ref_aux.view(sdt)).cuda()), (lib, lg, lgb, "aux")
    finally:
        del d, aux, ref, ref_aux
        _release(lib)


# ---------------------------------------------------------------- arguments outside the accepted range ----
@pytest.mark.parametrize("field", list(TWO_ADICITY))
def test_out_of_range_arguments_raise_before_any_transform(oracle, libs, field):
    """lg = 2-adicity + 1, order 4, and an LDE past the 2-adicity raise SpparkError on a small device tensor; a correct
    transform on the same context follows"""
    import torch
    import sppark_amd
    from sppark_amd import ffi
    O = oracle
    F = C.Field(O, field)
    L = ffi.load(field)
    w, lg = _w(field), 4
    x = F.from_ints([(3 ** i + i) % F.p for i in range(1 << lg)])
    d = torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if field == "bb31" else np.int64).reshape(-1)).cuda()
    torch.cuda.synchronize()
    for lgx, order in ((TWO_ADICITY[field] + 1, 1), (lg, 4)):
        with pytest.raises(ffi.SpparkError):
            ffi.check(L, L.compute_ntt(0, d.data_ptr(), lgx, order, 0, 0))
    with pytest.raises(ffi.SpparkError):
        ffi.check(L, L.sppark_lde(0, d.data_ptr(), 2, TWO_ADICITY[field] - 1, None, None))
    sppark_amd.compute_ntt(0, d, NR, 0, 0, field)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint32 if field == "bb31" else np.uint64).reshape(x.shape)
    assert (got == F.ntt(x, NR, 0, 0)).all(), field
    del d
    _release(field)
