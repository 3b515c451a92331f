"""Host model of the multilinear-table calls (include/sppark_amd_mle.h): pure Python integers on the wire format, never the
code under test.  Wire formats come from test_field_inverse_gpu.Info and test_field_arith_gpu.Arith; elements are handled
as field VALUES (Montgomery words taken out of Montgomery form; a tuple of four for the BabyBear quartic extension), and
the map between canonical wire rows and values is a bijection, so a value has one bit pattern.

The extension's product is re-derived here -- F_p[x] / (x^4 - beta), beta = -11 -- and tests/test_mle_model.py checks it
against the oracle's on a handful of pairs."""
import numpy as np

from test_field_arith_gpu import Arith

LOW, HIGH = 0, 1
PRODUCT, EQ_MUL_SUB = "product", "eq_mul_sub"
X4_BETA = -11


class Model:
    def __init__(self, field):
        self.field, self.ar = field, Arith(field)
        self.f = f = self.ar.f
        self.p, self.x4 = f.p, self.ar.x4
        self.zero = (0, 0, 0, 0) if self.x4 else 0
        self.one = (1, 0, 0, 0) if self.x4 else 1

    # ---- wire rows <-> values ----
    def vals(self, rows):
        ar, p = self.ar, self.p
        rows = self.f.rows(np.asarray(rows))
        if self.x4:
            return [tuple(int(c) * ar.rinv % p for c in r) for r in rows]
        return [v * ar.rinv % p for v in ar.ints(rows)]

    def rows(self, vals):
        ar, p = self.ar, self.p
        if self.x4:
            return np.array([[c * ar.R % p for c in v] for v in vals], dtype=self.f.dtype).reshape(-1, 4)
        return ar.rows([v * ar.R % p for v in vals])

    def row(self, val):
        return self.rows([val])[0]

    # ---- the field ----
    def add(self, a, b):
        if self.x4:
            return tuple((x + y) % self.p for x, y in zip(a, b))
        return (a + b) % self.p

    def sub(self, a, b):
        if self.x4:
            return tuple((x - y) % self.p for x, y in zip(a, b))
        return (a - b) % self.p

    def mul(self, a, b):
        p = self.p
        if not self.x4:
            return a * b % p
        c = [0] * 7
        for i in range(4):
            for j in range(4):
                c[i + j] += a[i] * b[j]
        return tuple((c[k] + (X4_BETA * c[k + 4] if k < 3 else 0)) % p for k in range(4))

    def smul(self, k, a):
        """an integer times an element"""
        if self.x4:
            return tuple(k * x % self.p for x in a)
        return k * a % self.p

    def line(self, lo, hi, r):
        return self.add(lo, self.mul(r, self.sub(hi, lo)))

    def total(self, vals):
        s = self.zero
        for v in vals:
            s = self.add(s, v)
        return s

    # ---- the calls ----
    @staticmethod
    def pairs(t, order):
        h = len(t) // 2
        return [(t[2 * i], t[2 * i + 1]) for i in range(h)] if order == LOW else [(t[i], t[i + h]) for i in range(h)]

    def fold(self, t, r, order):
        return [self.line(lo, hi, r) for lo, hi in self.pairs(t, order)]

    def evaluate(self, t, point):
        """f~(point): variable 0 first (each LOW fold makes variable j + 1 the new variable j)"""
        assert len(t) == 1 << len(point)
        for r in point:
            t = self.fold(t, r, LOW)
        return t[0]

    def eq(self, point):
        t = [self.one]
        for r in point:                                     # variable j is index bit j: the new bit goes on top
            hi = [self.mul(x, r) for x in t]
            t = [self.sub(x, y) for x, y in zip(t, hi)] + hi
        return t

    def eq_at(self, point, i):
        v = self.one
        for j, r in enumerate(point):
            v = self.mul(v, r if (i >> j) & 1 else self.sub(self.one, r))
        return v

    def form(self, form, fs):
        if form == EQ_MUL_SUB:
            e, a, b, c = fs
            return self.mul(e, self.sub(self.mul(a, b), c))
        v = fs[0]
        for x in fs[1:]:
            v = self.mul(v, x)
        return v

    def degree(self, form, ntables):
        return 3 if form == EQ_MUL_SUB else ntables

    def pair_terms(self, form, los, his):
        """the contribution of one pair of every table to s(0) .. s(d), by the DEFINITION f(t) = lo + t (hi - lo)"""
        d = self.degree(form, len(los))
        return [self.form(form, [self.add(lo, self.smul(t, self.sub(hi, lo))) for lo, hi in zip(los, his)]) for t in range(d + 1)]

    def round(self, tables, form, order):
        d = self.degree(form, len(tables))
        ps = [self.pairs(t, order) for t in tables]
        s = [self.zero] * (d + 1)
        for i in range(len(ps[0])):
            terms = self.pair_terms(form, [p[i][0] for p in ps], [p[i][1] for p in ps])
            s = [self.add(x, y) for x, y in zip(s, terms)]
        return s

    def full_sum(self, tables, form):
        return self.total(self.form(form, [t[i] for t in tables]) for i in range(len(tables[0])))

    def lagrange(self, s, r):
        """the polynomial of degree len(s) - 1 through (t, s[t]) at r"""
        p, d = self.p, len(s) - 1
        acc = self.zero
        for t in range(d + 1):
            num, den = self.one, 1
            for u in range(d + 1):
                if u != t:
                    num = self.mul(num, self.sub(r, self.smul(u, self.one)))
                    den = den * (t - u) % p
            acc = self.add(acc, self.mul(self.smul(pow(den, -1, p), s[t]), num))
        return acc

    def random_rows(self, n, seed):
        """n canonical wire rows"""
        f = self.f
        rng = np.random.default_rng(seed)
        if f.wide:
            x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
            x[:, 3] &= np.uint64(0x0fffffffffffffff)            # < 2^252 < every modulus
            return x
        return rng.integers(0, f.p, size=(n, f.w), dtype=np.uint64).astype(f.dtype)
