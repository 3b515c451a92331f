"""CPU: the host model of the FRI calls (tests/fri_model.py) against itself and the oracle: its domain is the oracle's
transform of X, a fold of the evaluations of random coefficients is the evaluations of c[2k] + beta c[2k+1], arity a is a single
folds, and the two orders agree under the bit-reversal permutation."""
import numpy as np
import pytest

import fri_model as FM

FIELDS = ["gl64", "bb31", "bb31x4", "bls12_381", "bn254"]


def _coeffs(m, n, seed):
    return m.vals(m.random_rows(n, seed))


@pytest.mark.parametrize("field", FIELDS)
def test_domain_is_a_coset_of_the_group_of_order_n(oracle, field):
    m = FM.FriModel(field)
    for lg in (0, 1, 2, 5):
        xs = m.domain(lg)
        assert xs[0] == 1 and len(set(xs)) == 1 << lg
        assert all(pow(x, 1 << lg, m.p) == 1 for x in xs)
        if lg:
            assert xs[1 << (lg - 1)] == m.p - 1 and xs[2 % len(xs)] == xs[1] * xs[1] % m.p       # x_i = w^i
        assert m.domain(lg, order=FM.BITREV) == FM.permute(xs, lg)
        g = m.coset_shift()
        assert g not in (0, 1) and m.domain(lg, "coset") == [g * x % m.p for x in xs]
    # the oracle's own Coset transform puts X on shift * w^i
    assert list(FM._oracle_x(m.base_field, 4, True)) == m.domain(4, "coset")


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("order", [FM.NATURAL, FM.BITREV])
def test_fold_is_the_coefficient_identity(oracle, field, order):
    m = FM.FriModel(field)
    for lg, shift in ((1, None), (3, None), (6, "coset"), (5, 12345)):
        c = _coeffs(m, 1 << lg, 7 + lg)
        beta = _coeffs(m, 1, 99)[0]
        ev = m.evaluate_poly(c, m.domain(lg, shift, order))
        for a in range(1, min(lg, 3) + 1):
            got = m.fold(ev, a, beta, shift, order)
            s = m.shift_value(shift)
            want = m.evaluate_poly(m.fold_coeffs(c, a, beta), m.domain(lg - a, pow(s, 1 << a, m.p), order))
            assert got == want, (field, lg, a, shift)


@pytest.mark.parametrize("field", FIELDS)
def test_arity_is_single_folds_and_the_orders_agree(oracle, field):
    m = FM.FriModel(field)
    lg = 6
    ev = _coeffs(m, 1 << lg, 3)
    beta = _coeffs(m, 1, 5)[0]
    for shift in (None, "coset"):
        s = m.shift_value(shift)
        for a in (1, 2, 3):
            step, b, sh = ev, beta, s
            for _ in range(a):
                step = m.fold(step, 1, b, sh, FM.NATURAL)
                b, sh = m.mul(b, b), sh * sh % m.p
            nat = m.fold(ev, a, beta, shift, FM.NATURAL)
            assert nat == step
            rev = m.fold(FM.permute(ev, lg), a, beta, shift, FM.BITREV)
            assert rev == FM.permute(nat, lg - a)


def test_reduce_base_is_the_lifted_matrix(oracle):
    m = FM.FriModel("bb31x4")
    cols = [[(7 * j + i * i) % m.p for i in range(8)] for j in range(5)]
    w = _coeffs(m, 5, 1)
    sub, prev = _coeffs(m, 1, 2)[0], _coeffs(m, 8, 3)
    lifted = [[m.embed(v) for v in col] for col in cols]
    assert m.reduce(cols, w, sub, prev, base=True) == m.reduce(lifted, w, sub, prev)
    assert (np.array(m.rows(m.reduce(cols, w, base=True))) < m.p).all()
