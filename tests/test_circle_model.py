"""CPU: the host model of the circle transform (tests/circle_model.py) against the definition it was written from, and
against the committed direct-definition vectors (tests/golden/circle_golden.json)."""
import json
import os

import numpy as np
import pytest

import circle_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def _rand(rng, *shape):
    return rng.integers(0, M.P, size=shape, dtype=np.uint32)


def test_generator_has_order_2_31():
    x, y = M.G
    assert (x * x + y * y) % M.P == 1
    assert M.gpow(1 << 31) == (1, 0)
    assert M.gpow(1 << 30) == (M.P - 1, 0)              # the only element of order 2: G^(2^30) != 1
    assert M.g_of_order(2) == (0, M.P - 1)
    assert M.g_of_order(3) == (32768, 2147450879)


def test_anchors():
    assert M.domain_direct(1) == [(0, 2147483646), (0, 1)]
    assert M.domain_direct(2) == [(32768, 2147450879), (2147450879, 32768), (32768, 32768), (2147450879, 2147450879)]
    assert M.direct_evaluate([1, 2, 3, 4], 2) == [32767, 2147450878, 163843, 2147319810]
    assert M.direct_evaluate(list(range(1, 9)), 3) == [885347334, 714723476, 1262332919, 1432563561, 2092305986, 1109642644,
                                                       55636419, 1037382257]
    assert M.forward(np.arange(1, 9, dtype=np.uint32), 3, M.NATURAL).tolist() == M.direct_evaluate(list(range(1, 9)), 3)


def test_golden_vectors():
    with open(os.path.join(HERE, "golden", "circle_golden.json")) as f:
        g = json.load(f)
    assert g["generator"] == list(M.G) and g["modulus"] == M.P
    for case in g["cases"]:
        k, c = case["lg"], np.array(case["coefficients"], dtype=np.uint32)
        assert M.domain(k, M.NATURAL).tolist() == case["domain_natural"]
        assert M.forward(c, k, M.NATURAL).tolist() == case["evals_natural"], k
        assert M.forward(c, k, M.BITREV).tolist() == case["evals_bitrev"], k
        assert M.inverse(np.array(case["evals_bitrev"], dtype=np.uint32), k, M.BITREV).tolist() == case["coefficients"]
        assert M.inverse(np.array(case["evals_natural"], dtype=np.uint32), k, M.NATURAL).tolist() == case["coefficients"]
    assert g["anchors"]["evals_1234_lg2"] == [32767, 2147450878, 163843, 2147319810]


@pytest.mark.parametrize("k", range(0, 9))
def test_fast_model_equals_the_definition(k):
    rng = np.random.default_rng(k)
    c = _rand(rng, 1 << k)
    want = M.direct_evaluate(c, k)
    assert M.forward(c, k, M.NATURAL).tolist() == want
    assert M.forward(c, k, M.BITREV).tolist() == [want[M.bitrev(q, k)] for q in range(1 << k)]
    assert M.domain(k).tolist() == [list(p) for p in M.domain_direct(k)]
    pos = np.arange(1 << k)
    nz = [int(j) for j in np.nonzero(c)[0][:5]]
    sparse = np.zeros(1 << k, dtype=np.uint32)
    sparse[nz] = c[nz]
    for order in (M.BITREV, M.NATURAL):
        assert (M.sparse_evaluate(nz, c[nz], k, pos, order) == M.forward(sparse, k, order)).all()


@pytest.mark.parametrize("k", range(0, 17))
def test_inverse_of_forward_is_the_identity(k):
    rng = np.random.default_rng(40 + k)
    c = _rand(rng, 2, 1 << k)
    for order in (M.BITREV, M.NATURAL):
        assert (M.inverse(M.forward(c, k, order), k, order) == c).all()
        assert (M.forward(M.inverse(c, k, order), k, order) == c).all()


def test_lde_is_the_padded_polynomial_on_the_larger_domain():
    rng = np.random.default_rng(77)
    for k in range(0, 6):
        for b in range(1, 4):
            c = _rand(rng, 1 << k)
            e = M.forward(c, k, M.NATURAL)
            coeffs, ext = M.lde(e, k, b, M.NATURAL)
            assert (coeffs == c).all()
            assert ext.tolist() == M.direct_evaluate(list(c) + [0] * ((1 << (k + b)) - (1 << k)), k + b)
            cb, eb = M.lde(M.forward(c, k, M.BITREV), k, b, M.BITREV)
            assert (cb == c).all() and [int(eb[q]) for q in range(1 << (k + b))] == [int(ext[M.bitrev(q, k + b)]) for q in range(1 << (k + b))]


def test_domains_are_distinct_and_disjoint():
    for k in range(1, 12):
        a = {tuple(p) for p in M.domain(k).tolist()}
        b = {tuple(p) for p in M.domain(k + 1).tolist()}
        assert len(a) == 1 << k and len(b) == 2 << k
        assert all((x * x + y * y) % M.P == 1 for x, y in a)
        assert not (a & b)
        assert not (a & {tuple(p) for p in M.domain(k + 2).tolist()})
