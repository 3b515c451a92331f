"""Host model of the FRI calls (include/sppark_amd_fri.h): pure Python integers on the wire format, built on mle_model.Model,
never the code under test.

The domain is NOT a constant copied from the library: its points are the oracle's transform of the polynomial X -- the
evaluations of X are the x_i -- in the order asked for; the coset generator is the oracle's Coset transform of X at its
first point.  Elements are field VALUES as in mle_model; the points of the domain are values of the BASE field (for the
BabyBear quartic extension: BabyBear integers, embedded in component 0 where an element is needed)."""
import functools

import numpy as np

from mle_model import Model

NATURAL, BITREV = 0, 1
BASE_OF = {"bb31x4": "bb31"}
VARIANT = {"gl64_plonky2": dict(goldilocks_plonky2=True), "bb31_canonical": dict(baby_bear_canonical=True)}
TWO_ADICITY = {"gl64": 32, "bb31": 27, "bb31x4": 27, "bls12_381": 32, "bn254": 28, "bls12_377": 47, "pallas": 32, "vesta": 32,
               "gl64_plonky2": 32, "bb31_canonical": 27}


def bitrev(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def permute(vals, lg):
    """natural order <-> bit-reversed order (an involution)"""
    return [vals[bitrev(i, lg)] for i in range(1 << lg)]


@functools.lru_cache(maxsize=None)
def _oracle_x(field, lg, coset):
    """the oracle's transform of X over 2^lg points, natural order, as values of |field| (a transform field)"""
    import oracle as O
    m = Model(field)
    f = m.f
    n = 1 << lg
    x = np.zeros((n, f.w), dtype=f.dtype)
    x[1] = f.one
    typ = O.COSET if coset else O.STANDARD
    kw = VARIANT.get(field)
    if kw:
        O.set_root_conventions(**kw)
    try:
        if f.oname == "gl64":
            y = O.ntt_gl64(x.reshape(-1), O.NN, O.FORWARD, typ).reshape(-1, 1)
        elif f.oname == "bb31":
            y = O.ntt_bb31(x.reshape(-1), O.NN, O.FORWARD, typ).reshape(-1, 1)
        else:
            y = O.ntt_fr(O.CURVE_ID[f.oname], x, O.NN, O.FORWARD, typ)
    finally:
        if kw:
            O.set_root_conventions()
    return tuple(m.vals(y))


class FriModel(Model):
    def __init__(self, field):
        super().__init__(field)
        self.base_field = BASE_OF.get(field, field)
        self.base = Model(self.base_field) if self.x4 else self
        self.inv2 = pow(2, -1, self.p)

    # ---- the domain: base-field integers ----
    def coset_shift(self):
        return _oracle_x(self.base_field, 1, True)[0]

    def shift_value(self, shift):
        """None, "coset" or a base-field value"""
        if shift is None:
            return 1
        return self.coset_shift() if isinstance(shift, str) else shift

    def domain(self, lg_n, shift=None, order=NATURAL):
        xs = list(_oracle_x(self.base_field, lg_n, False)) if lg_n else [1]
        s = self.shift_value(shift)
        xs = [x * s % self.p for x in xs]
        return permute(xs, lg_n) if order == BITREV else xs

    def embed(self, x):
        return (x % self.p, 0, 0, 0) if self.x4 else x % self.p

    def domain_minus(self, lg_n, shift, order, z=None):
        """the elements x_i - z"""
        return [self.sub(self.embed(x), z if z is not None else self.zero) for x in self.domain(lg_n, shift, order)]

    # ---- fold ----
    def fold_once(self, vals, xs, beta, order):
        """(the n / 2 folded values, the points of the squared domain in the same order)"""
        h = len(vals) // 2
        idx = [(k, k + h) for k in range(h)] if order == NATURAL else [(2 * k, 2 * k + 1) for k in range(h)]
        out = []
        for lo_i, hi_i in idx:
            lo, hi, x = vals[lo_i], vals[hi_i], xs[lo_i]
            assert (xs[hi_i] + x) % self.p == 0                     # the pair sits at x and -x
            even = self.smul(self.inv2, self.add(lo, hi))
            odd = self.smul(pow(2 * x, -1, self.p), self.sub(lo, hi))
            out.append(self.add(even, self.mul(beta, odd)))
        return out, [xs[lo_i] * xs[lo_i] % self.p for lo_i, _ in idx]

    def fold(self, vals, lg_arity, beta, shift=None, order=NATURAL):
        """lg_arity single folds with beta, beta^2, beta^4"""
        lg_n = len(vals).bit_length() - 1
        xs = self.domain(lg_n, shift, order)
        for _ in range(lg_arity):
            vals, xs = self.fold_once(vals, xs, beta, order)
            beta = self.mul(beta, beta)
        return vals

    def fold_coeffs(self, coeffs, lg_arity, beta):
        """the folded polynomial: c[2k] + beta c[2k+1], lg_arity times with beta, beta^2, beta^4"""
        for _ in range(lg_arity):
            coeffs = [self.add(coeffs[2 * k], self.mul(beta, coeffs[2 * k + 1])) for k in range(len(coeffs) // 2)]
            beta = self.mul(beta, beta)
        return coeffs

    def evaluate_poly(self, coeffs, xs):
        """the polynomial at the base-field points xs (Horner)"""
        out = []
        for x in xs:
            acc = self.zero
            for c in reversed(coeffs):
                acc = self.add(self.smul(x, acc), c)
            out.append(acc)
        return out

    # ---- reduce ----
    def reduce(self, cols, weights, sub=None, prev=None, base=False):
        """cols[j][i]: element (j, i) of the matrix (base: values of the base field); out[i]"""
        n = len(cols[0])
        out = []
        for i in range(n):
            acc = prev[i] if prev is not None else self.zero
            for col, w in zip(cols, weights):
                acc = self.add(acc, self.smul(col[i], w) if base else self.mul(w, col[i]))
            out.append(self.sub(acc, sub) if sub is not None else acc)
        return out
