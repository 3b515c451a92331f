"""CPU: the closed forms of tests/golden/ntt_closed_form.py against the oracle's full transforms.

tests/test_ntt_range_gpu.py checks the transforms above the reference's range (Goldilocks 2^29 ... 2^32, BLS12-381 Fr 2^29
and 2^30) only through these formulas, so they are pinned here: for every field and all 16 (order, direction, type) modes at
lg 1 ... 12, with K = 1 (R = 0), K = 7 (R != 0 from lg 3) and K = n + 3 (Q = 0), the closed form equals the oracle's whole
output at every index, bit-reversed orders included.  The negative controls show that the same check rejects an output with
one element changed, a transform with w^3 in place of w, and an output with two indices 2^s apart swapped."""
import numpy as np
import pytest

import ntt_closed_form as C

FIELDS = ["gl64", "bb31"] + list(C.WIDE)


def _table(F, K, seed):
    """K random elements with 0, 1, p - 1 in front (raw words below p)"""
    rng = np.random.default_rng(seed)
    v = [0, 1, F.p - 1] + [int.from_bytes(rng.bytes(40), "little") % F.p for _ in range(max(0, K - 3))]
    return F.from_ints(v[:K])


@pytest.mark.parametrize("field", FIELDS)
def test_closed_form_equals_the_oracle_every_index(oracle, field):
    F = C.Field(oracle, field)
    for lg in range(1, 13):
        n = 1 << lg
        every = np.arange(n)
        for K in sorted({1, 7, n + 3}):                               # R = 0; R != 0 (lg > 2); Q = 0
            T = _table(F, K, 100 * lg + K)
            pc = C.Periodic(F, lg, T)
            for order, direction, typ in C.MODES:
                if order == C.RR and direction == 0 and typ == 1:
                    continue
                got = F.ntt(pc.input(order), order, direction, typ)
                exp = pc.values(order, direction, typ, every)
                assert not C.mismatches(F, exp, got), (field, lg, K, order, direction, typ)
        rng = np.random.default_rng(lg)
        sel = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, size=min(n, 6))]))
        sp = C.Sparse(F, lg, sel, _table(F, len(sel), 7 + lg))
        for order, direction, typ in C.MODES:
            got = F.ntt(sp.input(order), order, direction, typ)
            assert not C.mismatches(F, sp.values(order, direction, typ, every), got), (field, lg, "sparse", order, direction, typ)


def test_positions_cover_the_boundaries():
    lg = 20
    ps = set(C.positions(lg, 100, 1).tolist())
    assert {0, 63, (1 << lg) - 64, (1 << lg) - 1} <= ps
    for s in range(1, lg):
        assert {(1 << s) - 1, 1 << s, (1 << s) + 1, (1 << lg) - (1 << s)} <= ps, s


@pytest.mark.parametrize("field", ["gl64", "bb31", "bls12_381", "bn254"])
def test_closed_form_check_rejects_wrong_outputs(oracle, field):
    """negative controls: the check that passes the oracle's output fails a corrupted one"""
    F = C.Field(oracle, field)
    lg, K = 8, 7
    n = 1 << lg
    every = np.arange(n)
    pc = C.Periodic(F, lg, _table(F, K, 5))
    p = F.p
    for order, direction, typ in [(C.NN, 0, 0), (C.NR, 0, 0), (C.RN, 1, 0), (C.NN, 0, 1), (C.NR, 1, 1)]:
        exp = pc.values(order, direction, typ, every)
        good = F.ntt(pc.input(order), order, direction, typ)
        assert not C.mismatches(F, exp, good)
        # one element changed
        bad = F.to_ints(good)
        bad[77] = (bad[77] + 1) % p
        assert C.mismatches(F, exp, F.from_ints(bad)) == [77], (field, order, direction, typ)
        # two indices 2^s apart swapped (where they differ)
        for s in (0, 3, lg - 1):
            bad = F.to_ints(good)
            a = 5 if s < lg - 1 else 1
            assert bad[a] != bad[a + (1 << s)]
            bad[a], bad[a + (1 << s)] = bad[a + (1 << s)], bad[a]
            assert C.mismatches(F, exp, F.from_ints(bad)) == [a, a + (1 << s)], (field, s)
        # a transform with w^3 in place of w (an independent textbook DFT) differs from it at all but the j with w^3j = w^j
        w3 = pow(F.root(lg), 3, p)
        alt = C.Periodic(F, lg, pc.T, root=w3).values(order, direction, typ, every)
        x = F.to_ints(pc.input(order))
        k = C.bitrev(every, lg) if order == C.RN else every          # coefficient index of each stored position
        cw = pow(w3, -1, p) if direction else w3
        coef = [0] * n
        for pos, v in zip(every, x):
            coef[k[pos]] = v
        if direction == 0 and typ == 1:
            coef = [v * pow(F.g, i, p) % p for i, v in enumerate(coef)]
        jj = C._logical(lg, order, every)
        naive = [sum(c * pow(cw, i * int(j) % n, p) for i, c in enumerate(coef)) % p for j in jj]
        naive = C._post(F, lg, order, direction, typ, jj, naive)
        assert naive == alt, (field, order, direction, typ)               # (the helper's formula with w^3 == the DFT with w^3)
        assert len(C.mismatches(F, exp, F.from_ints(naive))) > n // 2, (field, order, direction, typ)
