"""Every NTT mode at every size regime of the NTT plans, and the LDE over its (domain, blow-up) range, against the oracle.

The step sequence of the Goldilocks / BabyBear transforms is a function of lg (ntt_r64_kernels.hpp make_r64_plan: a
generic top pass over k_ntt12 for lg 13 ... 23 except 18, k_ntt6 on top at 18 and 24, two steps above k_ntt12 from 21),
and the coset multiplier is folded into the tables, over a generic top pass with row constants (r64_coset_mode).  The
256-bit fields run k_ntt_pass_lat's plan.  A root or coset generator that forward and inverse share passes every round
trip, so every (order, direction, type) is compared with the oracle here, at every lg of the plans' range.

The oracle is called once per (lg, direction, type) in NN order; NR is its output bit-reversed, RN the kernel's input
bit-reversed, standard RR is NN on the same array (ntt/ntt.cuh: NTT_RR == NTT_NN).  Coset RR multiplies position i by
g^bitrev(i) before a transform that reads position i as index i -- its exponents follow neither index -- so it is called
directly.  test_order_derivation (CPU) pins the derivation against direct oracle calls.  The oracle runs in threads (the
library releases the GIL) ahead of the GPU checks."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import recipe

SMALL = ["gl64", "bb31"]
WIDE = ["bls12_381", "bn254", "bls12_377", "pallas", "vesta"]
NN, NR, RN, RR = 0, 1, 2, 3
LGS = {"gl64": range(1, 24), "bb31": range(1, 24), "bls12_381": range(1, 21), "bn254": range(1, 21),
       "bls12_377": range(13, 20, 2), "pallas": range(13, 20, 2), "vesta": range(13, 20, 2)}
THREADS = 8


def _oracle_fn(O, field):
    if field in WIDE:
        curve = O.CURVE_ID[field]
        return lambda x, order, direction, typ: O.ntt_fr(curve, x, order, direction, typ)
    return O.ntt_gl64 if field == "gl64" else O.ntt_bb31


def _bitrev(lg):
    i = np.arange(1 << lg, dtype=np.int64)
    r = np.zeros_like(i)
    for k in range(lg):
        r |= ((i >> k) & 1) << (lg - 1 - k)
    return r


def _input(O, field, lg, seed):
    """uniform elements with the edges 0, 1, p - 1 in front (256-bit fields: (n, 4) u64 limbs of values < r, drawn
    in numpy with rejection -- recipe.ntt_input's big-int loop is too slow at 2^20)"""
    n = 1 << lg
    if field not in WIDE:
        x = recipe.ntt_input(field, lg, seed)
        p = O.GL64_P if field == "gl64" else O.BB31_P
        x[:min(n, 3)] = np.array([0, 1, p - 1], dtype=x.dtype)[:min(n, 3)]
        return x
    r = O.FR_MODULUS[O.CURVE_ID[field]]
    rl = [(r >> (64 * k)) & 0xffffffffffffffff for k in range(4)]
    top = np.uint64((1 << ((r.bit_length() - 1) % 64 + 1)) - 1)
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 4), dtype=np.uint64)
    bad = np.arange(n)
    while bad.size:
        y = rng.integers(0, 1 << 64, size=(bad.size, 4), dtype=np.uint64)
        y[:, 3] &= top
        lt = y[:, 0] < np.uint64(rl[0])
        for k in range(1, 4):
            lt = (y[:, k] < np.uint64(rl[k])) | ((y[:, k] == np.uint64(rl[k])) & lt)
        x[bad[lt]] = y[lt]
        bad = bad[~lt]
    for i, v in enumerate((0, 1, r - 1)[:n]):
        x[i] = [(v >> (64 * k)) & 0xffffffffffffffff for k in range(4)]
    return x


def _oracle_calls(f, x, submit):
    """the 6 oracle calls behind the 16 modes: NN of every (direction, type), coset RR of both directions"""
    calls = [(NN, d, t) for d in (0, 1) for t in (0, 1)] + [(RR, d, 1) for d in (0, 1)]
    return {c: submit(f, x, *c) for c in calls}


def _modes(x, lg, res):
    """{(order, direction, type): (kernel input, expected output)} for all 16 modes from the results of _oracle_calls"""
    rev = _bitrev(lg)
    out = {}
    for direction in (0, 1):
        for typ in (0, 1):
            nn = res[NN, direction, typ]
            out[NN, direction, typ] = (x, nn)
            out[NR, direction, typ] = (x, nn[rev])
            out[RN, direction, typ] = (x[rev], nn)
            out[RR, direction, typ] = (x, nn) if typ == 0 else (x, res[RR, direction, typ])
    return out


def test_order_derivation(oracle):
    """CPU: the NR / RN / RR derivation of _modes equals direct oracle calls (lg <= 10, every field)"""
    O = oracle
    for field in SMALL + WIDE:
        f = _oracle_fn(O, field)
        for lg in range(1, 11):
            x = _input(O, field, lg, 50 + lg)
            for (order, direction, typ), (xin, exp) in _modes(x, lg, _oracle_calls(f, x, lambda g, *a: g(*a))).items():
                assert (exp == f(xin, order, direction, typ)).all(), (field, lg, order, direction, typ)


@pytest.mark.gpu
@pytest.mark.parametrize("field", SMALL + WIDE)
def test_ntt_plan_ladder_all_modes_vs_oracle(oracle, libs, field):
    """all 4 orders x 2 directions x 2 types at every lg of the field's ladder, host buffers, whole outputs"""
    import sppark_amd
    O = oracle
    f = _oracle_fn(O, field)
    with ThreadPoolExecutor(THREADS) as ex:
        jobs = []
        for lg in LGS[field]:
            x = _input(O, field, lg, 1000 + lg)
            jobs.append((lg, x, _oracle_calls(f, x, ex.submit)))
        for lg, x, calls in jobs:
            for (order, direction, typ), (xin, exp) in _modes(x, lg, {c: j.result() for c, j in calls.items()}).items():
                y = xin.copy()
                sppark_amd.compute_ntt(0, y, order, direction, typ, field)
                assert y.shape == exp.shape and (y == exp).all(), (field, lg, order, direction, typ)


def _lde_cases(field):
    if field in SMALL:
        return [(lg, lgb) for lgb in (1, 2, 3) for lg in range(13 - lgb, 23 - lgb)]
    return [(lg, lgb) for lgb in (1, 2, 3) for lg in range(13 - lgb, 19 - lgb)]


@pytest.mark.gpu
@pytest.mark.parametrize("field", SMALL + ["bls12_381", "bn254"])
def test_lde_plan_ladder_vs_oracle(oracle, libs, field):
    """sppark_lde (the spread and coset shift fused into the first k_ntt12) with the coefficient output, every
    (lg_domain, lg_blowup in 1 ... 3) with 13 <= lg_domain + lg_blowup <= 22 (256-bit fields: <= 18), host buffers; the
    largest extension of every blow-up once more on device tensors."""
    import torch
    import sppark_amd
    O = oracle
    dt = np.uint32 if field == "bb31" else np.uint64
    sdt, tdt = (np.int32, torch.int32) if field == "bb31" else (np.int64, torch.int64)
    w = 4 if field in WIDE else 1
    cases = _lde_cases(field)
    top = {lgb: max(lg for lg, b in cases if b == lgb) for lgb in (1, 2, 3)}

    def expected(lg, lgb):
        x = _input(O, field, lg, 3000 + 8 * lg + lgb)
        return (x,) + O.lde(field, x, lgb, want_aux=True)

    with ThreadPoolExecutor(THREADS) as ex:
        jobs = [(lg, lgb, ex.submit(expected, lg, lgb)) for lg, lgb in cases]
        for lg, lgb, job in jobs:
            x, exp, aux_exp = job.result()
            buf = np.zeros((1 << (lg + lgb), w), dtype=dt); buf[:1 << lg] = x.reshape(-1, w)
            aux = np.zeros((1 << lg, w), dtype=dt)
            sppark_amd.LDE(0, buf, lg, lgb, field, aux_out=aux)
            assert (buf.reshape(exp.shape) == exp).all(), (field, lg, lgb)
            assert (aux.reshape(aux_exp.shape) == aux_exp).all(), (field, lg, lgb)
            if lg == top[lgb]:
                d = torch.zeros((1 << (lg + lgb)) * w, dtype=tdt, device="cuda")
                d[:(1 << lg) * w] = torch.from_numpy(np.ascontiguousarray(x).view(sdt).reshape(-1)).cuda()
                d_aux = torch.zeros((1 << lg) * w, dtype=tdt, device="cuda")
                sppark_amd.LDE(0, d, lg, lgb, field, aux_out=d_aux, stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert (d.cpu().numpy().view(dt).reshape(exp.shape) == exp).all(), (field, lg, lgb, "device")
                assert (d_aux.cpu().numpy().view(dt).reshape(aux_exp.shape) == aux_exp).all(), (field, lg, lgb, "device")
