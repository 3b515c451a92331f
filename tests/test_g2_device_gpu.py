"""GPU: the G2 arithmetic and every product form of the bucket field AS THE DEVICE EXECUTES THEM, operation by operation
(the hooks of csrc/api/devtest_g2_api.hip), against exact references: Python integers and the oracle's group law.  No
tolerance anywhere.  What the G2 MSM tests run end to end on random points is run here on the operands random points
never produce:

  * all seven product forms of ff/montx_dev.hpp (the asm statements of ff/montx_blocks.hpp) limb for limb against the
    column model of tests/montx_model.py, on the operands of the host test -- for the G1 bucket field of all five curves
    and for the base field of the G2 bucket field (ten 28-bit limbs over alt_bn128, an instantiation only G2 has);
  * ff/fp2x_dev.hpp at the edge of its bounds, and the Fp2 values with a vanishing component;
  * ff/fp2_dev.hpp (the loader's and the wire form's type) against Python integers, byte for byte;
  * the point operations of ec/xyzzx2_dev.hpp and ec/xyzz_dev.hpp over Fp2 on true G2 points (oracle) and on edge-valued
    coordinates (the EFD formulas on Python integers), with the rows in which a difference vanishes in ONE component;
  * the wave-pair bucket of ec/xyzz2_coop.hpp against the serial class, bit for bit, with the special cases meeting in
    one work-group, the vote all-true in one group and false in the next, and a ragged last group."""
import random

import numpy as np
import pytest

import montx_model
import recipe

pytestmark = pytest.mark.gpu
FEATURE = {"bls12_381": "BLS12_381", "bn254": "BN254", "bls12_377": "BLS12_377", "pallas": "PALLAS", "vesta": "VESTA"}
ALL_CURVES = ["bls12_381", "bn254", "bls12_377", "pallas", "vesta"]
G2_CURVES = ["bls12_381", "bn254", "bls12_377"]
LB = 28                                                         # limb size of the G2 bucket field's base field


def P(a):
    return a.ctypes.data


class Field:
    """the numbers of one curve's Fp2 = Fp[u] / (u^2 + NR) in its two device representations"""
    def __init__(self, O, name):
        self.name = name
        self.g1, self.g2 = O.CURVE_ID[name], O.CURVE_ID_G2[name]
        self.p = O.FP_MODULUS[self.g1]
        self.nb = O.FP_BYTES[self.g1]                           # bytes of a base-field element on the wire
        self.NL = (self.p.bit_length() + 8 + LB - 1) // LB      # internal limbs (ff/montx_dev.hpp: HEAD = 8)
        self.R = 1 << (LB * self.NL)                            # internal Montgomery radix
        self.Rw = 1 << (8 * self.nb)                            # the wire form's
        self.Rwinv = pow(self.Rw, -1, self.p)
        self.NR = 5 if name == "bls12_377" else 1
        self.one = self.Rw % self.p                             # 1 on the wire

    # ---- internal limbs (2 NL words per Fp2 element) ----
    def limbs(self, v):
        out = [(v >> (LB * j)) & ((1 << LB) - 1) for j in range(self.NL - 1)] + [v >> (LB * (self.NL - 1))]
        assert out[-1] < (1 << 31)
        return out

    def pack(self, els):
        return np.array([self.limbs(c0) + self.limbs(c1) for c0, c1 in els], dtype=np.uint32)

    def val(self, l):
        return sum(int(x) << (LB * j) for j, x in enumerate(l))

    def unpack(self, arr):
        a = arr.reshape(-1, 2, self.NL)
        assert (a[:, :, :self.NL - 1] < (1 << LB)).all(), "limbs not normalised"
        return [(self.val(e[0]), self.val(e[1])) for e in a]

    # ---- wire bytes (c0 | c1, canonical Montgomery images) ----
    def wire(self, rows):
        """rows of base-field integers -> (n, len(row) * nb) bytes"""
        return np.frombuffer(b"".join(int(v).to_bytes(self.nb, "little") for r in rows for v in r), dtype=np.uint8).reshape(len(rows), -1).copy()

    def unwire(self, arr):
        a = np.ascontiguousarray(arr).reshape(arr.shape[0], -1, self.nb)
        return [[int.from_bytes(c.tobytes(), "little") for c in r] for r in a]

    # ---- Fp2 on Montgomery images (Python integers) ----
    def mul(self, a, b):
        return ((a[0] * b[0] - self.NR * a[1] * b[1]) * self.Rwinv % self.p, (a[0] * b[1] + a[1] * b[0]) * self.Rwinv % self.p)

    def add(self, a, b):
        return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)

    def sub(self, a, b):
        return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)

    def neg(self, a):
        return (-a[0] % self.p, -a[1] % self.p)


def fp2_shapes(p, NR, rng, nrandom):
    """Fp2 values whose products and squares have a vanishing component, and pairs (a, b) with c0 = 0 or c1 = 0"""
    a, b, t = rng.randrange(1, p), rng.randrange(1, p), rng.randrange(2, p)
    shapes = [(0, 0), (1, 0), (0, 1), (p - 1, p - 1), (a, 0), (0, a), (a, a), (a, p - a), (b, a), (p - 1, 1)]
    shapes += [(rng.randrange(p), rng.randrange(p)) for _ in range(nrandom)]
    pairs = [(x, y) for x in shapes for y in shapes]
    for x in shapes:
        pairs.append((x, (x[0], -x[1] % p)))                                    # the conjugate: c1 = 0
        pairs.append((x, (NR * x[1] * t % p, x[0] * t % p)))                    # a0 b0 = NR a1 b1: c0 = 0
        pairs.append(((NR * x[1] * t % p, x[0] * t % p), x))
    return shapes, pairs


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [(c, 0) for c in ALL_CURVES] + [(c, 1) for c in G2_CURVES])
def test_block_forms_equal_the_column_model_on_device(libs, name, which):
    """operator*, mul2 (fat / normalised / mixed left operands), mul_add, sqr2 and sqr on raw limbs, one element per lane:
    r0, r1 are the column model's limbs EXACTLY, on the operands of tests/test_montx_blocks.py -- left limbs 2^31 - 1,
    MA_A0 2^LB - 1 and MA_A1 2^LB - 1 for mul_add, SQR_L 2^LB - 1 for sqr, the alternating patterns, all-ones normalised
    limbs, 0, 1, p - 1, p, 2p - 1, every left edge against every right edge, then random; n = 160 per form."""
    from sppark_amd import ffi
    L = ffi.load_devtest(name)
    inf = np.zeros(64, dtype=np.int32)
    assert L.sppark_devtest_blocks_info(which, P(inf)) == 0
    NL, LBITS = int(inf[0]), int(inf[1])
    assert (NL, LBITS) == montx_model.LIMBS[(FEATURE[name], which)]
    if name == "bn254" and which == 1:
        assert (NL, LBITS) == (10, 28)                          # the instantiation that exists for G2 only

    def run(form, A0, B0, A1, B1):
        r0 = np.full_like(A0, 0xa5a5a5a5); r1 = np.full_like(A0, 0xa5a5a5a5)
        ffi.check(L, L.sppark_devtest_blocks_run(which, form, P(r0), P(r1), P(A0), P(B0), P(A1), P(B1), A0.shape[0]))
        return r0, r1
    montx_model.check_forms(run, inf, (name, which), random.Random(1000 * which + NL))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G2_CURVES)
def test_fp2x_at_the_edge_of_its_bounds_on_device(oracle, libs, name):
    """ff/fp2x_dev.hpp on the device, on internal limbs.  For KA in {3, 6, 10, 13}: mul<KA> / sqr<KA> with the left (the
    square's) operand x + (KA - 2) p -- the largest normalised representative below (KA - 1) p -- and canonical, right
    operands up to 15 p, on the cases of the host test (test_fp2_over_the_lazy_field_at_the_edge_of_its_bounds) and on
    the Fp2 shapes random coordinates never have: a zero component, c0 = +-c1, conjugate pairs, pairs whose product has
    c0 = 0 or c1 = 0.  Against Python integers: c0 R = a0 b0 - NR a1 b1, c1 R = a0 b1 + a1 b0 (mod p), results below 2 p,
    limbs normalised; sub<KA> / neg<KA> with the subtrahend at its bound and (a + b).norm() exact as integers.
    is_zero_mod<KMAX>, KMAX in {5, 9, 10, 12}, component-wise: every (k p, k' p), k p +- 1, (k p, non-zero), (non-zero, k p).
    from_std then to_std is the identity on canonical input; to_std of any admissible lazy value is the canonical value."""
    from sppark_amd import ffi
    F = Field(oracle, name)
    L = ffi.load_devtest(name)
    p, NR, R, NL = F.p, F.NR, F.R, F.NL
    rng = random.Random(7 + F.g2)

    def run(op, ka, A, B=None):
        out = np.full_like(A, 0xa5a5a5a5)
        ffi.check(L, L.sppark_devtest_fp2x_op(op, ka, P(out), P(A), P(B if B is not None else A), A.shape[0]))
        return out

    for ka in (3, 6, 10, 13):
        edge = (ka - 2) * p
        _shapes, pairs = fp2_shapes(p, NR, rng, 3)
        xs, ys = [], []
        for i, (x, y) in enumerate(pairs):                      # left: canonical and lifted to the bound, component by component
            lift = [(0, 0), (edge, edge), (edge, 0), (0, edge)][i % 4]
            xs.append((x[0] + lift[0], x[1] + lift[1]))
            ys.append((y[0] + (i % 14) * p, y[1] + (13 - i % 14) * p))          # right operands up to 15 p
        # the rows of the host test
        xs += [(edge, edge), (p - 1 + edge, p - 1 + edge), (edge, p - 1 + edge)]
        ys += [(15 * p - 1, 15 * p - 1), (0, 0), (rng.randrange(p) + 13 * p, rng.randrange(p))]
        while len(xs) < 256:
            k = len(xs)
            xs.append((rng.randrange(p) + edge, rng.randrange(p) + edge))
            ys.append((rng.randrange(p) + (k % 14) * p, rng.randrange(p) + (13 - k % 14) * p))
        n = len(xs)
        assert 256 <= n < 400
        A, B = F.pack(xs), F.pack(ys)
        zero_c0 = zero_c1 = 0                                   # products with a vanishing component of two NON-ZERO operands
        nz = lambda v: v[0] % p != 0 or v[1] % p != 0
        for (a0, a1), (b0, b1), (c0, c1) in zip(xs, ys, F.unpack(run(0, ka, A, B))):
            assert (c0 * R - (a0 * b0 - NR * a1 * b1)) % p == 0 and (c1 * R - (a0 * b1 + a1 * b0)) % p == 0, ("mul", ka, a0 // p, a1 // p)
            assert c0 < 2 * p and c1 < 2 * p, ("mul bound", ka, c0 // p, c1 // p)
            if nz((a0, a1)) and nz((b0, b1)):
                zero_c0 += c0 % p == 0; zero_c1 += c1 % p == 0
        # (12 non-zero shapes: each with its conjugate gives c1 = 0, each on either side of its a0 b0 = NR a1 b1 partner c0 = 0)
        assert zero_c0 >= 24 and zero_c1 >= 12
        for (a0, a1), (c0, c1) in zip(xs, F.unpack(run(1, ka, A))):
            assert (c0 * R - (a0 * a0 - NR * a1 * a1)) % p == 0 and (c1 * R - 2 * a0 * a1) % p == 0, ("sqr", ka)
            assert c0 < 2 * p and c1 < 2 * p, ("sqr bound", ka)
        # a - b with b at its bound (< (KA - 1) p), a anything normalised below 15 p
        for (b0, b1), (a0, a1), (c0, c1) in zip(ys, xs, F.unpack(run(2, ka, B, A))):
            assert c0 == b0 + ka * p - a0 and c1 == b1 + ka * p - a1, ("sub", ka)
        for (a0, a1), (c0, c1) in zip(xs, F.unpack(run(3, ka, A))):
            assert c0 == ka * p - a0 and c1 == ka * p - a1, ("neg", ka)
        for (a0, a1), (b0, b1), (c0, c1) in zip(xs, ys, F.unpack(run(4, 0, A, B))):
            assert c0 == a0 + b0 and c1 == a1 + b1, ("add", ka)
        # to_std of a lazy value: v 2^(32 NW) / 2^(LB NL) mod p, canonical
        SH = LB * NL - 8 * F.nb
        got = F.unwire(np.ascontiguousarray(run(7, 0, A)[:, :2 * F.nb // 4]).view(np.uint8))
        for (a0, a1), (w0, w1) in zip(xs, got):
            assert (w0 << SH) % p == a0 % p and (w1 << SH) % p == a1 % p and w0 < p and w1 < p, ("to_std", ka)

    # to_std of un-normalised limbs (every limb but the top at 2^31 - 1: the left operand of a product)
    ptop = F.limbs(p)[NL - 1]
    fat = [[(1 << 31) - 1] * (NL - 1) + [ptop], [0] * NL, [(1 << 31) - 1 if j % 2 else 0 for j in range(NL - 1)] + [ptop]]
    fat += [[rng.randrange(1 << 31) for _ in range(NL - 1)] + [rng.randrange(ptop + 1)] for _ in range(61)]
    A = np.array([fat[i] + fat[(i + 1) % len(fat)] for i in range(len(fat))], dtype=np.uint32)
    SH = LB * NL - 8 * F.nb
    got = F.unwire(np.ascontiguousarray(run(7, 0, A)[:, :2 * F.nb // 4]).view(np.uint8))
    for i, (w0, w1) in enumerate(got):
        assert (w0 << SH) % p == F.val(fat[i]) % p and (w1 << SH) % p == F.val(fat[(i + 1) % len(fat)]) % p and w0 < p and w1 < p, ("to_std fat", i)

    # from_std: canonical wire words -> normalised, < 2 p, congruent to w 2^SH; and back
    ws = [(0, 0), (1, 0), (0, 1), (p - 1, p - 1), (F.one, p - F.one), ((1 << (p.bit_length() - 1)), (1 << (p.bit_length() - 1)) - 1)]
    ws += [(rng.randrange(p), rng.randrange(p)) for _ in range(250)]
    W = np.zeros((len(ws), 2 * NL), dtype=np.uint32)
    W[:, :2 * F.nb // 4] = F.wire(ws).view(np.uint32)
    internal = run(6, 0, W)
    for (w0, w1), (c0, c1) in zip(ws, F.unpack(internal)):
        assert c0 < 2 * p and c1 < 2 * p and c0 % p == (w0 << SH) % p and c1 % p == (w1 << SH) % p, "from_std"
    back = run(7, 0, internal)
    assert (back[:, :2 * F.nb // 4] == W[:, :2 * F.nb // 4]).all() and (back[:, 2 * F.nb // 4:] == 0).all()

    for kmax in (5, 9, 10, 12):                                  # (10: what the mixed additions ask of R, 9 p included)
        vals = [(k * p, k2 * p) for k in range(kmax) for k2 in range(kmax)]
        for k in range(kmax):
            r = rng.randrange(1, p) + rng.randrange(kmax) * p   # non-zero mod p, below KMAX p
            vals += [(k * p + 1, k * p), (k * p, k * p + 1), (k * p + 1, k * p + 1), (k * p, r), (r, k * p), (r, r)]
            vals += [(k * p + 1, ((k + 1) % kmax) * p), (((k + 2) % kmax) * p, k * p + 1)]
            if k:
                vals += [(k * p - 1, k * p), (k * p, k * p - 1), (k * p - 1, 0), (0, k * p - 1)]
        assert all(c0 < kmax * p and c1 < kmax * p for c0, c1 in vals)
        out = run(5, kmax, F.pack(vals))
        expect = np.array([int(c0 % p == 0 and c1 % p == 0) for c0, c1 in vals], dtype=np.uint32)
        assert expect.sum() == kmax * kmax
        assert (out[:, 0] == expect).all(), (kmax, np.nonzero(out[:, 0] != expect)[0][:8])
        assert (out[:, 1:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G2_CURVES)
def test_wire_fp2_class_against_python_integers(oracle, libs, name):
    """ff/fp2_dev.hpp over the canonical 32-bit-limb class (the point loader's type): +, -, *, sqr, neg, dbl on the wire
    bytes of ~2048 pairs -- the shapes with a zero component, c0 = +-c1, conjugates and the pairs whose product has a
    vanishing component, then random -- byte for byte what Python integers give on the Montgomery images."""
    from sppark_amd import ffi
    F = Field(oracle, name)
    L = ffi.load_devtest(name)
    p = F.p
    rng = random.Random(70 + F.g2)
    _shapes, pairs = fp2_shapes(p, F.NR, rng, 30)
    while len(pairs) < 2048:
        pairs.append(((rng.randrange(p), rng.randrange(p)), (rng.randrange(p), rng.randrange(p))))
    xs, ys = [a for a, _ in pairs], [b for _, b in pairs]
    A, B = F.wire(xs), F.wire(ys)
    ref = {0: [F.add(a, b) for a, b in pairs], 1: [F.sub(a, b) for a, b in pairs], 2: [F.mul(a, b) for a, b in pairs],
           3: [F.mul(a, a) for a in xs], 4: [F.neg(a) for a in xs], 5: [F.add(a, a) for a in xs]}
    nzp = [c for (a, b), c in zip(pairs, ref[2]) if a != (0, 0) and b != (0, 0)]     # products of two non-zero operands
    assert sum(c[0] == 0 for c in nzp) >= 78 and sum(c[1] == 0 for c in nzp) >= 39      # (39 non-zero shapes, as above)
    for op in range(6):
        out = np.full_like(A, 0xa5)
        ffi.check(L, L.sppark_devtest_fp2_wire_op(op, P(out), P(A), P(B), A.shape[0]))
        want = F.wire(ref[op])
        bad = np.nonzero((out != want).any(axis=1))[0]
        assert bad.size == 0, (name, op, int(bad[0]), xs[bad[0]], ys[bad[0]])


# ---------------------------------------------------------------------------------------------------------------------
def _xyzz_op(ffi, L, impl, op, xa, operand):
    out = np.full_like(xa, 0xa5)
    ffi.check(L, L.sppark_devtest_g2_xyzz_op(impl, op, P(out), P(xa), P(operand) if operand is not None else 0, xa.shape[0]))
    return out


@pytest.mark.parametrize("name", G2_CURVES)
def test_g2_point_operations_against_the_oracle(oracle, libs, name):
    """add / madd / madd of the negative / dbl of xyzz_dev<fp2_dev> (impl 0) and xyzz_dev<fp2x_dev> (impl 1) on true G2
    points, n = 96 (not a multiple of 64), accumulators with ZZ, ZZZ != 1 (two mixed additions first), with the rows: equal
    operands (XYZZ-equal for add, the accumulator's own affine point for madd), opposite operands, operand at infinity,
    accumulator at infinity, both at infinity.  Expected: the oracle's Jacobian addition / doubling over the G2 curve,
    compared as affine points; and the two classes agree bit for bit (they evaluate the same formulas in every branch)."""
    from sppark_amd import ffi
    O = oracle
    F = Field(O, name)
    L = ffi.load_devtest(name)
    g2, fb2, n = F.g2, 2 * F.nb, 96
    A = O.g1_gen_points(g2, n, 11)
    xa = np.zeros((n, 4 * fb2), dtype=np.uint8)
    xa[:, :2 * fb2] = A
    xa[:, 2 * fb2:] = F.wire([[F.one, 0, F.one, 0]])[0]
    for seed in (13, 14):                                       # ZZ, ZZZ != 1
        xa = _xyzz_op(ffi, L, 0, 1, xa, O.g1_gen_points(g2, n, seed))
    xb = _xyzz_op(ffi, L, 0, 1, xa, O.g1_gen_points(g2, n, 15))
    xb = _xyzz_op(ffi, L, 0, 1, xb, O.g1_gen_points(g2, n, 16))
    B = O.g1_gen_points(g2, n, 12)

    def negated(y_bytes):
        return F.wire([[-v % F.p for v in F.unwire(y_bytes.reshape(1, -1))[0]]])[0]
    xb[0] = xa[0]                                               # equal XYZZ operands: the doubling inside add
    B[0] = O.xyzz_to_affine(g2, xa[0])                          # the accumulator's own point: the doubling inside madd (op 1)
    xb[1] = xa[1]; xb[1, fb2:2 * fb2] = negated(xa[1, fb2:2 * fb2])             # opposite
    B[1] = O.xyzz_to_affine(g2, xa[1]); B[1, fb2:] = negated(B[1, fb2:])
    B[5] = O.xyzz_to_affine(g2, xa[5]); B[5, fb2:] = negated(B[5, fb2:]); B[6] = O.xyzz_to_affine(g2, xa[6])     # (the same two for op 2)
    xb[2] = 0; B[2] = 0                                         # operand at infinity
    xa[3] = 0                                                   # accumulator at infinity
    xa[4] = 0; xb[4] = 0; B[4] = 0                              # both
    xa[70] = 0; xb[71] = 0; B[71] = 0                           # (and in the second, partial work-group)

    def jac(aff):                                               # affine (all-zero: infinity) -> Jacobian
        j = np.zeros(3 * fb2, dtype=np.uint8)
        if aff.any():
            j[:2 * fb2] = aff; j[2 * fb2:] = F.wire([[F.one, 0]])[0]
        return j
    Bneg = B.copy()
    for i in range(n):
        if B[i].any():
            Bneg[i, fb2:] = negated(B[i, fb2:])
    acc_aff = [O.xyzz_to_affine(g2, xa[i]) for i in range(n)]
    oth_aff = [O.xyzz_to_affine(g2, xb[i]) for i in range(n)]
    for op, operand in ((0, xb), (1, B), (2, B), (3, None)):
        got0, got1 = _xyzz_op(ffi, L, 0, op, xa, operand), _xyzz_op(ffi, L, 1, op, xa, operand)
        for i in range(n):
            ja = jac(acc_aff[i])
            want = O.jac_dbl(g2, ja) if op == 3 else O.jac_add(g2, ja, jac(oth_aff[i] if op == 0 else B[i] if op == 1 else Bneg[i]))
            want = O.jac_to_affine(g2, want)
            assert (O.xyzz_to_affine(g2, got1[i]) == want).all(), (name, "lazy class", op, i)
            assert (O.xyzz_to_affine(g2, got0[i]) == want).all(), (name, "wire class", op, i)
        assert (got0 == got1).all(), (name, op, np.nonzero((got0 != got1).any(axis=1))[0][:8])
        # the special rows did what they are there for
        inf = lambda r: not r[2 * fb2:].any()
        if op == 0:
            assert inf(got1[1]) and not inf(got1[0]) and (got1[2] == xa[2]).all() and (got1[3] == xb[3]).all() and inf(got1[4])
        if op == 1:
            assert inf(got1[1]) and not inf(got1[0]) and (got1[2] == xa[2]).all() and inf(got1[4]) and inf(got1[5]) and not inf(got1[6])
        if op == 2:
            assert inf(got1[0]) and inf(got1[6]) and not inf(got1[1]) and not inf(got1[5])


# ---------------------------------------------------------------------------------------------------------------------
class EFD:
    """madd-2008-s, add-2008-s, dbl-2008-s-1 and mdbl-2008-s-1 over Fp2 on Python integers (Montgomery images in, Montgomery
    images out), with the branch structure of the device classes: P = 0 and R = 0 is a doubling, P = 0 and R != 0 infinity.
    A point is (X, Y, ZZZ, ZZ), each an Fp2 pair; None is infinity."""
    def __init__(self, F):
        self.F = F

    def dbl(self, a):
        if a is None:
            return None
        F = self.F
        X, Y, ZZZ, ZZ = a
        U = F.add(Y, Y); V = F.mul(U, U); W = F.mul(U, V); S = F.mul(X, V)
        M = F.mul(X, X); M = F.add(F.add(M, M), M)
        X3 = F.sub(F.sub(F.mul(M, M), S), S)
        Y3 = F.sub(F.mul(M, F.sub(S, X3)), F.mul(W, Y))
        return (X3, Y3, F.mul(ZZZ, W), F.mul(ZZ, V))

    def madd(self, a, q, negate):
        F = self.F
        if q is None:
            return a
        x, y = q
        if negate:
            y = F.neg(y)
        one = (F.one, 0)
        if a is None:
            return (x, y, one, one)
        X, Y, ZZZ, ZZ = a
        Pd = F.sub(F.mul(x, ZZ), X); Rd = F.sub(F.mul(y, ZZZ), Y)
        if Pd != (0, 0):
            PP = F.mul(Pd, Pd); PPP = F.mul(Pd, PP); Q = F.mul(X, PP)
            X3 = F.sub(F.sub(F.sub(F.mul(Rd, Rd), PPP), Q), Q)
            Y3 = F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(Y, PPP))
            return (X3, Y3, F.mul(ZZZ, PPP), F.mul(ZZ, PP))
        if Rd == (0, 0):
            return self.dbl((x, y, one, one))                   # mdbl-2008-s-1: dbl-2008-s-1 with ZZ = ZZZ = 1
        return None

    def add(self, a, b):
        F = self.F
        if b is None:
            return a
        if a is None:
            return b
        X, Y, ZZZ, ZZ = a
        U1 = F.mul(X, b[3]); S1 = F.mul(Y, b[2])
        Pd = F.sub(F.mul(b[0], ZZ), U1); Rd = F.sub(F.mul(b[1], ZZZ), S1)
        if Pd != (0, 0):
            PP = F.mul(Pd, Pd); PPP = F.mul(Pd, PP); Q = F.mul(U1, PP)
            X3 = F.sub(F.sub(F.sub(F.mul(Rd, Rd), PPP), Q), Q)
            Y3 = F.sub(F.mul(Rd, F.sub(Q, X3)), F.mul(S1, PPP))
            return (X3, Y3, F.mul(F.mul(ZZZ, PPP), b[2]), F.mul(F.mul(ZZ, PP), b[3]))
        if Rd == (0, 0):
            return self.dbl(a)
        return None


@pytest.mark.parametrize("name", G2_CURVES)
def test_g2_point_operations_on_edge_valued_coordinates(oracle, libs, name):
    """The point formulas over Fp2 on coordinates that are edge values of the field (no curve needed: the formulas are
    polynomial identities), n = 512, each COMPONENT drawn 70 % from the field's edge values and 30 % at random, with the
    forced rows in which the zero tests of the branches see ONE vanishing component, or a component that is zero on
    both sides of a difference: U2 - X (madd) and U2 - U1 (add) zero
    in c0 only, in c1 only, and zero in both with S2 - Y (S2 - S1) zero in exactly one component -- that is infinity, not a
    doubling -- beside the true doublings and the operands at infinity.  Reference: class EFD above, on the canonical
    values.  X, Y, ZZZ, ZZ must be exactly those values from the lazy class (impl 1) AND from the wire class (impl 0), in
    every row: both classes evaluate the same formula in every branch (the doubling inside add doubles the XYZZ
    accumulator in both, the one inside madd is mdbl of the affine operand in both), so no branch is compared as
    x = X / ZZ, y = Y / ZZZ instead and no row is left out for either.
    (The accumulator's Y is kept non-zero in Fp2: Y = 0 would be a point of order two, which these groups do not have, and
    the two classes are not required to agree on doubling it.  ZZ and ZZZ are kept non-zero likewise -- only an all-zero
    ZZZ | ZZ is infinity.)"""
    from sppark_amd import ffi
    F = Field(oracle, name)
    L = ffi.load_devtest(name)
    E = EFD(F)
    p, NL = F.p, F.NL
    rng = random.Random(500 + F.g2)
    edge = [0, 1, 2, p - 1, p - 2, F.Rw % p, (F.Rw - 1) % p, (p - 1) // 2, (1 << LB) - 1, ((1 << (LB * (NL - 1))) - 1) % p, (1 << 31) - 1]
    m = 512

    def fp2(nonzero=False):
        v = tuple(rng.choice(edge) if rng.random() < 0.7 else rng.randrange(p) for _ in range(2))
        return (1, 0) if nonzero and v == (0, 0) else v
    # rows of Fp2 pairs: accumulator, XYZZ operand, affine operand
    acc = [[fp2(), fp2(True), fp2(True), fp2(True)] for _ in range(m)]
    oth = [[fp2(), fp2(), fp2(True), fp2(True)] for _ in range(m)]
    aff = [[fp2(), fp2()] for _ in range(m)]
    one = (F.one, 0)
    d = lambda v, k: (v[0] + (k == 0), v[1] + (k == 1))        # move one component off
    for r, comp in ((20, 1), (21, 0)):                          # madd: U2 - X vanishes in c0 only / in c1 only
        acc[r][0] = tuple(c % p for c in d(F.mul(aff[r][0], acc[r][3]), comp))
    for r, neg, comp in ((22, 0, 1), (23, 0, 0), (24, 1, 1), (25, 1, 0), (26, 0, None), (27, 1, None)):
        # U2 - X = 0 with +-S2 - Y zero in exactly one component (infinity), or in both (26, 27: the doubling), for op 1 / op 2
        aff[r][1] = fp2(True)
        acc[r][0] = F.mul(aff[r][0], acc[r][3])
        s2 = F.mul(F.neg(aff[r][1]) if neg else aff[r][1], acc[r][2])
        acc[r][1] = s2 if comp is None else tuple(c % p for c in d(s2, comp))
    for r, neg, y in ((28, 1, (0, rng.randrange(1, p))), (29, 1, (rng.randrange(1, p), 0)), (35, 0, (0, rng.randrange(1, p)))):
        # the doubling of -q where -S2 and Y are BOTH ZERO in one component (y has a zero component, ZZZ lies in Fp): the
        # difference is the largest value the lazy class's zero test of R ever sees, 3 p + 6 p - 0
        aff[r][1] = y
        acc[r][2] = (rng.randrange(1, p), 0)
        acc[r][0] = F.mul(aff[r][0], acc[r][3])
        acc[r][1] = F.mul(F.neg(y) if neg else y, acc[r][2])
        assert 0 in acc[r][1]
    for r, comp in ((30, 1), (31, 0), (32, 1), (33, 0), (34, None)):            # the same for add (ZZ2 = ZZZ2 = 1: U1 = X, S1 = Y)
        oth[r][2] = one; oth[r][3] = one
        u2, s2 = F.mul(oth[r][0], acc[r][3]), F.mul(oth[r][1], acc[r][2])
        if r in (30, 31):
            acc[r][0] = tuple(c % p for c in d(u2, comp))
        else:
            oth[r][1] = fp2(True); s2 = F.mul(oth[r][1], acc[r][2])
            acc[r][0] = u2
            acc[r][1] = s2 if comp is None else tuple(c % p for c in d(s2, comp))
    oth[13] = list(acc[13])                                     # equal XYZZ operands
    assert all(a[1] != (0, 0) and a[2] != (0, 0) and a[3] != (0, 0) for a in acc) and all(b[2] != (0, 0) and b[3] != (0, 0) for b in oth)
    inf_acc, inf_oth, inf_aff = {7, 15, 300}, {9, 15, 301}, {11, 15, 301}
    pa = [None if i in inf_acc else tuple(acc[i]) for i in range(m)]
    pb = [None if i in inf_oth else tuple(oth[i]) for i in range(m)]
    pq = [None if (i in inf_aff or aff[i] == [(0, 0), (0, 0)]) else tuple(aff[i]) for i in range(m)]
    flat = lambda pt, k: [0] * (2 * k) if pt is None else [c for e in pt for c in e]
    xa = F.wire([flat(a, 4) for a in pa]); xb = F.wire([flat(b, 4) for b in pb]); xq = F.wire([flat(q, 2) for q in pq])
    branches = set()
    for op, operand in ((0, xb), (1, xq), (2, xq), (3, None)):
        want = []
        for i in range(m):
            want.append(E.add(pa[i], pb[i]) if op == 0 else E.dbl(pa[i]) if op == 3 else E.madd(pa[i], pq[i], op == 2))
        want_w = F.wire([flat(w, 4) for w in want])
        for impl in (1, 0):
            got = _xyzz_op(ffi, L, impl, op, xa, operand)
            bad = np.nonzero((got != want_w).any(axis=1))[0]
            assert bad.size == 0, (name, "impl", impl, "op", op, "rows", bad[:8].tolist())
        # the forced rows take the branch they were built for
        if op == 0:
            assert want[30] is not None and want[31] is not None and want[32] is None and want[33] is None
            assert want[34] == E.dbl(pa[34]) and want[13] == E.dbl(pa[13]) and want[34] is not None
            branches.add("add")
        if op in (1, 2):
            assert want[20] is not None and want[21] is not None
            k = 0 if op == 1 else 2
            assert want[22 + k] is None and want[23 + k] is None
            for r in ((26, 35) if op == 1 else (27, 28, 29)):
                assert want[r] is not None and want[r] == E.dbl((pq[r][0], F.neg(pq[r][1]) if op == 2 else pq[r][1], one, one)), r
            branches.add("madd%d" % op)
    assert branches == {"add", "madd1", "madd2"}


# ---------------------------------------------------------------------------------------------------------------------
def _chain(ffi, L, impl, pts, entries, nlanes, steps, words, want_std):
    internal = np.full((steps * nlanes, words), 0xa5a5a5a5, dtype=np.uint32)
    std = np.full((steps * nlanes, pts_wire_bytes(pts) * 2), 0xa5, dtype=np.uint8) if want_std else None
    ent = np.ascontiguousarray(entries, dtype=np.uint32)
    ffi.check(L, L.sppark_devtest_g2_chain(impl, P(internal), P(std) if want_std else 0, P(pts), pts.shape[1], pts.shape[0],
                                           P(ent), nlanes, steps))
    return internal, std


def pts_wire_bytes(pts):
    return pts.shape[1] & ~15                                   # bytes of X | Y (the flagged layout adds 8)


def _bucket_invariant(F, internal):
    """all four coordinates normalised, X < 9 p, Y < 5 p, ZZZ, ZZ < 2 p, in both components (ec/xyzzx2_dev.hpp)"""
    NL = F.NL
    img = internal.reshape(-1, 4, 2, NL)
    assert (img < (1 << LB)).all(), "limbs not below 2^28"
    # value < K p  <=  compare limb vectors from the top: done on Python integers, one per coordinate component
    w = [1 << (LB * j) for j in range(NL)]
    vals = (img.astype(object) * np.array(w, dtype=object)).sum(axis=3)        # (rows, 4, 2) Python integers
    for k, bound in enumerate((9, 5, 2, 2)):
        assert (vals[:, k, :] < bound * F.p).all(), ("coordinate", k, "bound", bound)


@pytest.mark.parametrize("name", G2_CURVES)
def test_wave_pair_bucket_equals_the_serial_class_on_device(oracle, libs, name):
    """g2c_bucket::madd (two waves, five LDS slots, eight barriers, the work-group vote) against xyzz_dev<fp2x_dev>'s
    set / madd through sppark_devtest_g2_chain: 3 * 64 + 17 lanes, 8 steps, on the 70 flagged points of the recipe (one of
    them at infinity).  The work-groups differ: group 0 holds every special case at once (lane 3 meets its start point
    again, lane 5 its negative -- infinity, then a fresh start --, lane 7 starts on the point at infinity, lane 9 meets it
    mid-chain, lane 11 restarts at step 4); in group 1 EVERY lane doubles at step 1 (the vote is all-true); group 2 has no
    special lane (the vote is false); in the ragged last group one lane doubles at step 2 and another restarts and then
    doubles at step 5.  A second run uses off-curve records whose next point shares only X.c0, only X.c1, X and only
    Y.c0, or X and only Y.c1 with the accumulator after a set -- one component vanishes, the other does not -- and
    records with a zero component of Y that come twice with the same sign, and -- in every work-group, among the other
    lanes -- records (x, y) with a zero component of Y that are set without negation and then meet the subtraction of
    (x, -y): -S2 = 3 p and Y = 0 there, so that component of R is exactly 9 p and the result must be the doubling.
    Required: the wave pairs' internal images equal the serial class's bit for bit at every step and lane; every image
    satisfies the bucket invariant; on-curve, the last step equals the oracle's sum of the same signed points."""
    from sppark_amd import ffi
    O = oracle
    F = Field(O, name)
    L = ffi.load_devtest(name)
    g2, fb2 = F.g2, 2 * F.nb
    nlanes, steps = 3 * 64 + 17, 8
    words = 4 * 2 * F.NL
    pts, _sc = recipe.msm_inputs(g2, 70, 99, flagged=True)
    assert pts.shape == (70, 2 * fb2 + 8) and pts[3, 2 * fb2] == 1              # the point at infinity
    INF = 3
    # indices of distinct plain points: the recipe repeats its 64 points from index 64 on, 7 = 8, 12 = -1
    plain = [i for i in range(64) if i not in (INF, 7, 12)]
    ent = np.zeros((steps, nlanes), dtype=np.uint64)
    E = lambda idx, neg=0, restart=0: idx | (neg << 31) | (restart << 30)
    for l in range(nlanes):
        for s in range(steps):
            ent[s, l] = E(plain[(l + s) % len(plain)], (l + s) & 1, int(s == 0))
    NEG, RESTART = 1 << 31, 1 << 30
    ent[1, 3] = int(ent[0, 3]) & ~RESTART                       # group 0: the same point again
    ent[1, 5] = (int(ent[0, 5]) & ~RESTART) ^ NEG               # its negative: infinity; step 2 starts afresh (no restart flag)
    ent[0, 7] = E(INF, 0, 1)                                    # starts on the point at infinity
    ent[3, 9] = E(INF, 1, 0)                                    # meets it mid-chain
    ent[4, 11] = int(ent[4, 11]) | RESTART                      # restarts
    for l in range(64, 128):                                    # group 1: every lane doubles at step 1
        ent[1, l] = int(ent[0, l]) & ~RESTART
    l = 192 + 2                                                 # ragged group: doubles at step 2 ...
    ent[1, l] = E(plain[40], 1, 1); ent[2, l] = E(plain[40], 1, 0)
    l = 192 + 9                                                 # ... restarts at step 4 and doubles at step 5
    ent[4, l] = E(plain[41], 0, 1); ent[5, l] = E(plain[41], 0, 0)
    ent = ent.astype(np.uint32)

    ser, ser_std = _chain(ffi, L, 0, pts, ent, nlanes, steps, words, True)
    par, par_std = _chain(ffi, L, 1, pts, ent, nlanes, steps, words, True)
    bad = np.argwhere((ser != par).any(axis=1)).ravel()
    assert bad.size == 0, (name, "step, lane", [(int(b) // nlanes, int(b) % nlanes) for b in bad[:8]])
    assert (ser_std == par_std).all()
    _bucket_invariant(F, par)
    img = par.reshape(steps, nlanes, words)
    assert not img[1, 5].any() and img[2, 5].any() and not img[0, 7].any() and img[1, 7].any()      # infinity where it must be
    assert (img[3, 9] == img[2, 9]).all() and img[0].any(axis=1).sum() == nlanes - 1
    # the oracle's sum of the same signed points
    one2 = F.wire([[F.one, 0]])[0]
    last = par_std.reshape(steps, nlanes, 4 * fb2)[steps - 1]
    for l in range(nlanes):
        acc = np.zeros(3 * fb2, dtype=np.uint8)
        for s in range(steps):
            e = int(ent[s, l])
            if e & RESTART:
                acc[:] = 0
            idx = e & 0x3fffffff
            if idx == INF:
                continue
            j = np.zeros(3 * fb2, dtype=np.uint8)
            j[:2 * fb2] = pts[idx, :2 * fb2]; j[2 * fb2:] = one2
            if e & NEG:
                j[fb2:2 * fb2] = F.wire([[-v % F.p for v in F.unwire(j[fb2:2 * fb2].reshape(1, -1))[0]]])[0]
            acc = O.jac_add(g2, acc, j)
        assert (O.xyzz_to_affine(g2, last[l]) == O.jac_to_affine(g2, acc)).all(), (name, "lane", l)

    # ---- off-curve records: one component of a difference vanishes, the other does not ----
    rng = random.Random(900 + g2)
    base = pts[:, :2 * fb2].copy(); base[INF] = 0               # plain layout: infinity is all-zero
    comps = [F.unwire(base[i].reshape(1, -1))[0] for i in range(70)]            # X.c0, X.c1, Y.c0, Y.c1
    extra, starts, ent2 = [], [], np.zeros((steps, nlanes), dtype=np.uint64)
    kinds = {}
    for l in range(nlanes):
        start = plain[l % len(plain)]
        neg = neg1 = l & 1                                      # (the same sign at both steps: +-S2 meets +-Y)
        x0, x1, y0, y1 = comps[start]
        other = lambda v: (v + rng.randrange(1, F.p)) % F.p
        kind = l % 7
        if kind >= 5:                                           # the start point itself has Y.c0 = 0 (or Y.c1 = 0) ...
            start = 70 + nlanes + l
            x0, x1, y0, y1 = (x0, x1, 0, y1) if l & 2 else (x0, x1, y0, 0)
            starts.append([x0, x1, y0, y1])
            if kind == 6:                                       # ... is set WITHOUT negation (Y = 0 exactly there) ...
                neg, neg1 = 0, 1
        else:
            starts.append(comps[start])                         # (unused filler: keeps the record indices regular)
        q = {0: [x0, other(x1), other(y0), other(y1)],          # shares only X.c0
             1: [other(x0), x1, other(y0), other(y1)],          # only X.c1
             2: [x0, x1, y0, other(y1)],                        # X and only Y.c0: infinity, not a doubling
             3: [x0, x1, other(y0), y1],                        # X and only Y.c1
             4: comps[plain[(l + 1) % len(plain)]],             # (an ordinary next point)
             5: [x0, x1, y0, y1],                               # ... and comes again: +-S2 and Y are both 0 there -- a doubling
             # ... and its negative is SUBTRACTED: -S2 = neg<3>(0) = 3 p meets Y = 0, R = 3 p + 6 p - 0 = 9 p in that
             # component, the largest value the zero test of R sees -- a doubling, not infinity
             6: [x0, x1, -y0 % F.p, -y1 % F.p]}[kind]
        kinds[l] = kind
        extra.append(q)
        ent2[0, l] = E(start, neg, 1)
        ent2[1, l] = E(70 + l, neg1, 0)
        for s in range(2, steps):
            ent2[s, l] = E(plain[(l + s) % len(plain)], (l + s) & 1, 0)
    pts2 = np.concatenate([base, F.wire(extra), F.wire(starts)], axis=0)
    ent2 = ent2.astype(np.uint32)
    ser, _ = _chain(ffi, L, 0, pts2, ent2, nlanes, steps, words, False)
    par, _ = _chain(ffi, L, 1, pts2, ent2, nlanes, steps, words, False)
    bad = np.argwhere((ser != par).any(axis=1)).ravel()
    assert bad.size == 0, (name, "off-curve: step, lane, kind", [(int(b) // nlanes, int(b) % nlanes, kinds[int(b) % nlanes]) for b in bad[:8]])
    _bucket_invariant(F, par)
    img = par.reshape(steps, nlanes, words)
    for l in range(nlanes):
        assert img[0, l].any()
        assert img[1, l].any() == (kinds[l] not in (2, 3)), (name, "lane", l, "kind", kinds[l])      # infinity exactly there
