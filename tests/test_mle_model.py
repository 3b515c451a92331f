"""CPU: the host model of the multilinear-table calls (tests/mle_model.py) against the definitions of
include/sppark_amd_mle.h -- the model is what every other mle test compares with."""
import numpy as np
import pytest

import mle_model as M

FIELDS = ["gl64", "bb31", "m31", "bb31x4", "bls12_381"]
FORMS = [(M.PRODUCT, 1), (M.PRODUCT, 2), (M.PRODUCT, 3), (M.PRODUCT, 4), (M.EQ_MUL_SUB, 4)]


def _tables(m, lg, count, seed):
    return [m.vals(m.random_rows(1 << lg, seed + k)) for k in range(count)]


def test_extension_product_is_the_oracles(oracle):
    """the re-derived product of F_p[x] / (x^4 + 11) on wire rows, edge values included"""
    m = M.Model("bb31x4")
    f = m.f
    x, y = m.random_rows(12, 1), m.random_rows(12, 2)
    x[0], x[1], y[1], y[2] = f.one, f.pm1, f.pm1, 0
    x[3] = [0, 0, 0, f.p - 1]; y[3] = [0, 0, 0, f.p - 1]       # x^3 * x^3 = beta x^2
    want = m.ar.mul(x, y)
    got = m.rows([m.mul(a, b) for a, b in zip(m.vals(x), m.vals(y))])
    assert (got == want).all()


@pytest.mark.parametrize("field", FIELDS)
def test_rows_and_values_round_trip(oracle, field):
    m = M.Model(field)
    x = m.random_rows(9, 3)
    x[0], x[1], x[2] = 0, m.f.one, m.f.pm1
    assert (m.rows(m.vals(x)) == x).all()
    assert m.vals(x[:3]) == [m.zero, m.one, m.sub(m.zero, m.one)]


@pytest.mark.parametrize("field", FIELDS)
def test_evaluate_on_the_corners_returns_the_table(oracle, field):
    m = M.Model(field)
    for lg in range(0, 5):
        t = _tables(m, lg, 1, 10 + lg)[0]
        for i in range(1 << lg):
            corner = [m.one if (i >> j) & 1 else m.zero for j in range(lg)]
            assert m.evaluate(t, corner) == t[i], (field, lg, i)


@pytest.mark.parametrize("field", FIELDS)
def test_eq_dotted_with_the_table_is_evaluate(oracle, field):
    m = M.Model(field)
    for lg in range(0, 6):
        t, point = _tables(m, lg, 1, 20 + lg)[0], m.vals(m.random_rows(max(lg, 1), 30 + lg))[:lg]
        e = m.eq(point)
        assert len(e) == 1 << lg
        assert e == [m.eq_at(point, i) for i in range(1 << lg)], (field, lg)
        assert m.total(m.mul(a, b) for a, b in zip(t, e)) == m.evaluate(t, point), (field, lg)


@pytest.mark.parametrize("field", FIELDS)
def test_round_sums_and_folds_agree(oracle, field):
    """s(0) + s(1) is the full sum of the form, and s(r) -- by Lagrange interpolation -- is s'(0) + s'(1) of the tables
    folded by r: both orders, both forms, every table count"""
    m = M.Model(field)
    for lg in (1, 2, 4):
        for form, nt in FORMS:
            tables = _tables(m, lg, nt, 40 + 7 * lg + nt)
            r = m.vals(m.random_rows(1, 50 + lg))[0]
            for order in (M.LOW, M.HIGH):
                s = m.round(tables, form, order)
                assert len(s) == m.degree(form, nt) + 1
                assert m.add(s[0], s[1]) == m.full_sum(tables, form), (field, lg, form, nt, order)
                folded = [m.fold(t, r, order) for t in tables]
                assert all(len(t) == 1 << (lg - 1) for t in folded)
                if lg > 1:
                    s2 = m.round(folded, form, order)
                    assert m.add(s2[0], s2[1]) == m.lagrange(s, r), (field, lg, form, nt, order)
                assert m.full_sum(folded, form) == m.lagrange(s, r), (field, lg, form, nt, order)
                for t in range(len(s)):                         # the interpolation passes through its own nodes
                    assert m.lagrange(s, m.smul(t, m.one)) == s[t]


@pytest.mark.parametrize("field", FIELDS)
def test_fold_order_and_evaluate(oracle, field):
    """binding every variable by folds -- LOW takes variable 0 first, HIGH the last -- is evaluate at the point in that order"""
    m = M.Model(field)
    lg = 4
    t = _tables(m, lg, 1, 60)[0]
    point = m.vals(m.random_rows(lg, 61))
    lo, hi = t, t
    for j in range(lg):
        lo = m.fold(lo, point[j], M.LOW)
        hi = m.fold(hi, point[lg - 1 - j], M.HIGH)
    assert lo[0] == hi[0] == m.evaluate(t, point)
