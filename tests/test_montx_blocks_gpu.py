"""GPU: the column blocks of the bucket field's products (ff/montx_blocks.hpp) as the device executes them -- one asm
statement per column -- at the edges of their contracts, against the wire-format class (ff/mont_dev.hpp: canonical 32-bit
limbs, plain carry chains) and Python integers, for every curve (all bucket field classes use the blocks).

  * sppark_devtest_bucket_field_op on raw limbs: x * y with left limbs 2^31 - 1 and all-ones normalised right limbs, x.sqr()
    with limbs up to SQR_L 2^LB, zero, 1, p - 1, p, 2p - 1: to_std(result) is the wire class's product of to_std(x), to_std(y)
    (times the domain offset), and the raw limbs are normalised;
  * sppark_devtest_bucket_xyzz_op (mul2 with normalised / fat left operands, sqr2, mul_add inside add / madd / dbl) on
    accumulators and points whose coordinates are edge values of the field: bit for bit the wire class's result.
The host emulation of the same blocks, limb for limb: tests/test_montx_blocks.py."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CURVES = [(0, "bls12_381", 14, 28), (1, "bn254", 9, 29), (4, "bls12_377", 14, 28), (6, "pallas", 9, 29), (7, "vesta", 9, 29)]


def P(a):
    return a.ctypes.data


@pytest.mark.parametrize("curve,name,NL,LB", CURVES)
def test_block_products_at_the_edges_of_their_contracts(oracle, libs, curve, name, NL, LB):
    from sppark_amd import ffi
    O = oracle
    L = ffi.load_devtest(name)
    assert L.sppark_devtest_bucket_field_limbs() == NL
    p, nb = O.FP_MODULUS[curve], O.FP_BYTES[curve]
    NW = nb // 4
    MASK = (1 << LB) - 1
    SQR_L = 4 if LB == 28 else 2
    R = 1 << (LB * NL)
    Rinv = pow(R, -1, p)
    limbs = lambda v: [(v >> (LB * j)) & MASK if j < NL - 1 else v >> (LB * j) for j in range(NL)]
    val = lambda l: sum(int(x) << (LB * j) for j, x in enumerate(l))
    ptop = limbs(p)[NL - 1]
    rng = random.Random(curve)
    # every limb but the top at its bound, the top limb the modulus' own: the value stays below 2p + (the contract bounds both)
    const = lambda v: [v] * (NL - 1) + [ptop]

    def patterns(top):
        e = [const(top), [0] * NL, limbs(1), limbs(p - 1), limbs(p), limbs(2 * p - 1),
             [top if j % 2 else 0 for j in range(NL - 1)] + [ptop], [0 if j % 2 else top for j in range(NL - 1)] + [0]]
        return e
    fat, nrm, sq = patterns((1 << 31) - 1), patterns(MASK), patterns((SQR_L << LB) - 1)
    n = 1024

    def column(edges, top, normalised):
        rows = [edges[i % len(edges)] for i in range(n)]
        for i in range(len(edges) ** 2, n):
            rows[i] = limbs(rng.randrange(2 * p)) if normalised else [rng.randrange(top + 1) for _ in range(NL - 1)] + [rng.randrange(ptop + 1)]
        return rows
    x = column(fat, (1 << 31) - 1, False)
    y = [nrm[(i // len(fat)) % len(nrm)] for i in range(n)]           # every left edge against every right edge
    for i in range(len(fat) * len(nrm), n):
        y[i] = limbs(rng.randrange(2 * p))
    s = column(sq, (SQR_L << LB) - 1, False)
    X, Y, S = (np.array(v, dtype=np.uint32) for v in (x, y, s))

    def run(op, a, b):
        out = np.zeros((n, NL), dtype=np.uint32)
        ffi.check(L, L.sppark_devtest_bucket_field_op(op, P(out), P(a), P(b), n))
        return out

    def std(a):                                                 # any admissible lazy value -> canonical wire bytes
        return np.ascontiguousarray(run(6, a, a)[:, :NW]).view(np.uint8).reshape(-1)

    def wire(op, a, b):
        out = np.zeros_like(a)
        ffi.check(L, L.sppark_devtest_field_op(0, op, P(out), P(a), P(b), n))
        return out
    # the wire domain is x 2^(32 NW), the bucket field's x 2^(LB NL): to_std(x (*) y) = to_std(x) * to_std(y) in the wire class
    prod, sqr = run(0, X, Y), run(1, S, S)
    assert (prod[:, :NL - 1] <= MASK).all() and (sqr[:, :NL - 1] <= MASK).all()
    assert (std(prod) == wire(2, std(X), std(Y))).all(), name
    assert (std(sqr) == wire(3, std(S), std(S))).all(), name
    for i in range(n):                                          # and Python integers on the raw limbs
        assert val(prod[i]) % p == val(x[i]) * val(y[i]) * Rinv % p and val(prod[i]) <= val(x[i]) * val(y[i]) // R + p, (name, i)
        assert val(sqr[i]) % p == val(s[i]) ** 2 * Rinv % p, (name, i)

    # point operations on coordinates that are edge values of the field (no curve needed: both classes evaluate the same
    # formulas on the same field elements), fed and read back in the wire form
    one = O.field_op(O.FP_FIELD_ID[curve], 4, O.int_to_limbs(1, nb)).view(np.uint8)
    Rw = 1 << (8 * nb)
    edge = [0, 1, 2, p - 1, p - 2, Rw % p, (Rw - 1) % p, (p - 1) // 2, (1 << LB) - 1, ((1 << (LB * (NL - 1))) - 1) % p, (1 << 31) - 1]
    m = 512

    def coords(k, nonzero=False):
        vals = [rng.choice(edge) if rng.random() < 0.7 else rng.randrange(p) for _ in range(m)]
        if nonzero:
            vals = [v if v else 1 for v in vals]
        return np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in vals), dtype=np.uint8).reshape(m, nb).copy()
    # (the accumulator's Y is kept non-zero: Y = 0 would be a point of order two, which these curves' groups do not have, and
    # the two classes are not required to agree on doubling it -- the wire class and the lazy class differ there)
    xa = np.concatenate([coords(0), coords(1, True), coords(2, True), coords(3, True)], axis=1)
    xb = np.concatenate([coords(4), coords(5), coords(6, True), coords(7, True)], axis=1)
    aff = np.concatenate([coords(8, True), coords(9)], axis=1)
    xa[7] = 0; xb[9] = 0; aff[11] = 0                           # operands at infinity
    xb[13] = xa[13]                                             # equal operands
    for op, operand in ((0, xb), (1, aff), (2, aff), (3, None)):
        ref = np.zeros_like(xa); got = np.zeros_like(xa)
        ptr = P(operand) if operand is not None else 0
        ffi.check(L, L.sppark_devtest_xyzz_op(op, P(ref), P(xa), ptr, m))
        ffi.check(L, L.sppark_devtest_bucket_xyzz_op(op, P(got), P(xa), ptr, m))
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert bad.size == 0, (name, op, int(bad[0]))
