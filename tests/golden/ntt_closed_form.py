"""Expected NTT outputs at chosen indices, for inputs whose transform has a closed form at any index.

Used where no full reference transform fits (tests/test_ntt_range_gpu.py: Goldilocks 2^29 ... 2^32, BLS12-381 Fr 2^29 and
2^30) and pinned against the oracle's full transforms at every index in tests/test_ntt_closed_form.py.

Periodic input of odd period K: x_i = T[i mod K].  With n = QK + R (0 <= R < K) its polynomial is

    P(y) = G(y) (1 - y^(QK)) / (1 - y^K) + y^(QK) G_R(y),   G = sum_{m<K} T[m] y^m,   G_R = sum_{m<R} T[m] y^m,

(P(1) = (Q + 1) sum T[<R] + Q sum T[>=R]); 1 - y^K != 0 at every other point used here, because K is odd.  The modes follow
oracle/ntt.hpp (the reference's NTT_internal): with j the natural output index and w the 2^lg-th root,

    forward            P(w^j)                 forward coset       P(g w^j)
    inverse            n^-1 P(w^-j)           inverse coset       n^-1 g^-j P(w^-j)   (RR order: g^-rev(j))

NR writes index j at position rev(j), RN reads coefficient k from position rev(k), NN and RR are natural in and out.  The
forward coset RR transform multiplies position i by g^rev(i) (an exponent that follows neither index), so it has no closed
form on a periodic input; Sparse gives the exact output of an input with a few nonzero positions for every mode instead.

Arithmetic is on Python integers mod p.  The transform is linear, so the raw words of a Montgomery field (bb31, the 256-bit
fields) can be taken as plain field elements: raw output = NTT of the raw input with the plain roots.  G and G_R are
evaluated by oracle.poly_evaluate, fed y R mod p so that its Montgomery products return plain values.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NN, NR, RN, RR = 0, 1, 2, 3
WIDE = ("bls12_381", "bn254", "bls12_377", "pallas", "vesta")
MODES = [(o, d, t) for o in range(4) for d in range(2) for t in range(2)]


def bitrev(i, lg):
    """bit reversal of the lg-bit indices |i| (numpy int64 array)"""
    i = np.asarray(i, dtype=np.int64)
    r = np.zeros_like(i)
    for k in range(lg):
        r |= ((i >> k) & 1) << (lg - 1 - k)
    return r


class Field:
    """modulus, Montgomery factor, root and generator of one field, as plain integers"""

    def __init__(self, O, field):
        self.O, self.name = O, field
        self.wide = field in WIDE
        if self.wide:
            self.curve = O.CURVE_ID[field]
            self.p, self.mont, self.limbs, self.dtype = O.FR_MODULUS[self.curve], 1 << 256, 4, np.uint64
        elif field == "gl64":
            self.p, self.mont, self.limbs, self.dtype = O.GL64_P, 1, 1, np.uint64
        else:
            self.p, self.mont, self.limbs, self.dtype = O.BB31_P, 1 << 32, 1, np.uint32
        self.rinv = pow(self.mont % self.p, -1, self.p)
        # the coset generator as the oracle applies it: the forward coset transform of [0, 1] at 2^1 is [g, -g]
        self.g = self.to_ints(self.ntt(self.from_ints([0, 1]), NN, 0, 1))[0]

    def root(self, lg):
        """the 2^lg-th root of unity the forward transform uses"""
        L = self.O.lib()
        if self.wide:
            w = self.to_ints(self.O.fr_root(self.curve, lg).reshape(1, 4))[0]
        elif self.name == "gl64":
            w = int(L.oracle_gl64_root(lg))
        else:
            w = int(L.oracle_bb31_root(lg))
        return w * self.rinv % self.p                     # (raw -> plain)

    def ntt(self, x, order, direction, typ):
        O = self.O
        if self.wide:
            return O.ntt_fr(self.curve, x, order, direction, typ)
        return (O.ntt_gl64 if self.name == "gl64" else O.ntt_bb31)(x, order, direction, typ)

    def to_ints(self, a):
        a = np.asarray(a)
        if not self.wide:
            return [int(v) for v in a.reshape(-1)]
        a = a.reshape(-1, 4)
        return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]

    def from_ints(self, v):
        if not self.wide:
            return np.array(v, dtype=self.dtype)
        m = (1 << 64) - 1
        return np.array([[(x >> (64 * k)) & m for k in range(4)] for x in v], dtype=np.uint64).reshape(-1, 4)

    def poly(self, coeffs, ys, threads=1):
        """[sum_m coeffs[m] y^m for y in ys] (plain integers; coeffs: raw array, taken as plain integers)"""
        if len(coeffs) == 0 or len(ys) == 0:
            return [0] * len(ys)
        xs = self.from_ints([y * self.mont % self.p for y in ys])
        field = self.name

        def run(lo, hi):
            return self.to_ints(self.O.poly_evaluate(field, coeffs, xs[lo:hi]))
        step = -(-len(ys) // max(1, threads))
        if threads <= 1 or len(ys) < 64:
            return run(0, len(ys))
        with ThreadPoolExecutor(threads) as ex:             # (ctypes releases the GIL)
            parts = list(ex.map(lambda lo: run(lo, lo + step), range(0, len(ys), step)))
        return [v for part in parts for v in part]


def _points(F, lg, j, direction, typ, root=None):
    """evaluation point of natural output index j (list of ints)"""
    p = F.p
    w = root if root is not None else F.root(lg)
    if direction == 1:
        w = pow(w, -1, p)
    c = F.g if (direction == 0 and typ == 1) else 1
    return [c * pow(w, int(k), p) % p for k in j]


def _post(F, lg, order, direction, typ, j, vals):
    """inverse: n^-1 and, for the coset, g^-j (g^-rev(j) in the RR order)"""
    if direction == 0:
        return vals
    p, n = F.p, 1 << lg
    ninv = pow(n, -1, p)
    if typ == 0:
        return [v * ninv % p for v in vals]
    ginv = pow(F.g, -1, p)
    e = bitrev(j, lg) if order == RR else np.asarray(j)
    return [v * ninv % p * pow(ginv, int(k), p) % p for v, k in zip(vals, e)]


def _logical(lg, order, positions):
    """natural output index held at each storage position"""
    positions = np.asarray(positions, dtype=np.int64)
    return bitrev(positions, lg) if order == NR else positions


class Periodic:
    """x_i = T[i mod K] (natural index i; stored at position rev(i) for the RN order)"""

    def __init__(self, F, lg, T, root=None):
        self.F, self.lg, self.T = F, lg, np.ascontiguousarray(T)
        self.K = len(self.T) if not F.wide else self.T.shape[0]
        assert self.K % 2 == 1
        self.root = root                                     # (negative controls only: another root)
        n = 1 << lg
        self.Q, self.R = divmod(n, self.K)
        t = F.to_ints(self.T)
        self.sum_lo, self.sum_hi = sum(t[:self.R]) % F.p, sum(t[self.R:]) % F.p

    def input(self, order):
        """the whole stored input (small lg only)"""
        n = 1 << self.lg
        i = np.arange(n, dtype=np.int64)
        src = bitrev(i, self.lg) if order == RN else i
        return self.T[src % self.K]

    def P(self, ys, threads=1):
        F, p, K, Q, R = self.F, self.F.p, self.K, self.Q, self.R
        gr = F.poly(self.T[:R], ys, threads)
        h = F.poly(self.T[R:], ys, threads)                  # G = G_R + y^R H
        out = []
        for y, a, b in zip(ys, gr, h):
            if y == 1:
                out.append(((Q + 1) * self.sum_lo + Q * self.sum_hi) % p)
                continue
            yk = pow(y, K, p)
            assert yk != 1, "1 - y^K = 0: the closed form does not apply at this point"
            yqk = pow(yk, Q, p)
            g = (a + pow(y, R, p) * b) % p
            out.append((g * (1 - yqk) * pow(1 - yk, -1, p) + yqk * a) % p)
        return out

    def values(self, order, direction, typ, positions, threads=1):
        """expected outputs at the storage |positions| (plain integers)"""
        assert not (order == RR and direction == 0 and typ == 1), "forward coset RR: no closed form (use Sparse)"
        j = _logical(self.lg, order, positions)
        v = self.P(_points(self.F, self.lg, j, direction, typ, self.root), threads)
        return _post(self.F, self.lg, order, direction, typ, j, v)


class Sparse:
    """an input that is zero except at a few storage positions: the exact output of every mode at any index"""

    def __init__(self, F, lg, pos, vals):
        self.F, self.lg = F, lg
        self.pos = np.asarray(pos, dtype=np.int64)
        self.vals = F.to_ints(vals)

    def input(self, order):
        n = 1 << self.lg
        x = np.zeros((n, 4) if self.F.wide else n, dtype=self.F.dtype)
        x[self.pos] = self.F.from_ints(self.vals)
        return x

    def values(self, order, direction, typ, positions, threads=1):
        F, lg, p, n = self.F, self.lg, self.F.p, 1 << self.lg
        k = bitrev(self.pos, lg) if order == RN else self.pos      # coefficient index of each nonzero
        c = list(self.vals)
        if direction == 0 and typ == 1:                              # the forward coset factor: g^k, RR: g^rev(position)
            e = bitrev(self.pos, lg) if order == RR else k
            c = [v * pow(F.g, int(x), p) % p for v, x in zip(c, e)]
        w = F.root(lg)
        if direction == 1:
            w = pow(w, -1, p)
        j = _logical(lg, order, positions)
        v = [sum(cv * pow(w, int(kk) * int(jj) % n, p) for cv, kk in zip(c, k)) % p for jj in j]
        return _post(F, lg, order, direction, typ, j, v)


def positions(lg, nrand, seed, edge=64, per_boundary=3):
    """storage positions to check: the first and last |edge|, m 2^s - 1, m 2^s, m 2^s + 1 at every power of two 2^s (every
    pass boundary of any plan) for m = 1, 2, 3, the last and |per_boundary| random ones, and |nrand| uniform positions"""
    n = 1 << lg
    rng = np.random.default_rng(seed)
    ps = [np.arange(min(edge, n)), n - 1 - np.arange(min(edge, n))]
    for s in range(1, lg):
        top = n >> s
        ms = np.unique(np.concatenate([np.array([1, 2, 3, top - 1]), rng.integers(1, top, size=per_boundary)]))
        ms = ms[(ms >= 1) & (ms < top)]
        for d in (-1, 0, 1):
            ps.append((ms << s) + d)
    ps.append(rng.integers(0, n, size=nrand))
    out = np.unique(np.concatenate(ps).astype(np.int64))
    return out[(out >= 0) & (out < n)]


def mismatches(F, expected, observed):
    """indices where the raw |observed| array differs from the plain integers |expected|"""
    got = F.to_ints(observed)
    return [i for i, (e, g) in enumerate(zip(expected, got)) if e != g]
