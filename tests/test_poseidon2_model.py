"""CPU: the host model of Poseidon2 (tests/poseidon2_model.py) against the definition of include/sppark_amd_poseidon2.h taken
literally -- M_E and M_I as explicitly built T x T matrices, x^7 as pow, the sponge's permutations counted by hand -- the
batch form against the one-state form, and the package's own verifier (sppark_amd.poseidon2.verify, a second set of
Python-integer lines) against the model's trees: an honest path is accepted; a flipped bit, a wrong index and a swapped
sibling are not."""
import numpy as np
import pytest

import poseidon2_model as M

FIELDS = ("bb31", "gl64")
ROUNDS = {"bb31": ((2, 0), (8, 1), (8, 13)), "gl64": ((2, 0), (8, 1), (8, 22))}


def params(field, rf, rp, seed=0):
    from sppark_amd import poseidon2
    return poseidon2.test_params(field, rf, rp, seed)


def rand_state(field, rng, count=None):
    p, t = M.MODULUS[field], M.WIDTH[field]
    draw = lambda: int(rng.integers(0, 1 << 63)) * int(rng.integers(0, 1 << 63)) % p      # noqa: E731
    if count is None:
        return [draw() for _ in range(t)]
    return np.array([[draw() for _ in range(t)] for _ in range(count)], dtype=M.value_dtype(field))


def circ_external(t):
    """circ(2 M4, M4, .., M4) as a T x T matrix of integers"""
    big = [[0] * t for _ in range(t)]
    for bi in range(t // 4):
        for bj in range(t // 4):
            for i in range(4):
                for j in range(4):
                    big[4 * bi + i][4 * bj + j] = M.M4[i][j] * (2 if bi == bj else 1)
    return big


def matvec(mat, x, p):
    return [sum(mat[i][j] * x[j] for j in range(len(x))) % p for i in range(len(x))]


@pytest.mark.parametrize("field", FIELDS)
def test_linear_layers_are_the_explicit_matrices(field):
    p, t = M.MODULUS[field], M.WIDTH[field]
    rng = np.random.default_rng(1)
    me = circ_external(t)
    assert me[0][:8] == [4, 6, 2, 2, 2, 3, 1, 1] and me[5][:8] == [1, 2, 3, 1, 2, 4, 6, 2]
    d = rand_state(field, rng)
    mi = [[(d[i] if i == j else 0) + 1 for j in range(t)] for i in range(t)]              # diag(d) + the all-ones matrix
    edge = [[0] * t, [1] * t, [p - 1] * t] + [[(p - 1) if i == k else 0 for i in range(t)] for k in range(t)]
    for x in [rand_state(field, rng) for _ in range(20)] + edge:
        assert M.external(list(x), p) == matvec(me, x, p)
        assert M.internal(list(x), d, p) == matvec(mi, x, p)


@pytest.mark.parametrize("field", FIELDS)
def test_sbox_is_the_seventh_power_and_a_permutation_exponent(field):
    p = M.MODULUS[field]
    rng = np.random.default_rng(2)
    for x in [0, 1, 2, p - 1, p - 2] + rand_state(field, rng):
        assert M.sbox(x, p) == pow(x, 7, p)
    from math import gcd
    assert gcd(7, p - 1) == 1 and all(gcd(e, p - 1) != 1 for e in (2, 3, 4, 5, 6))
    assert (p - 1) in (15 << 27, (1 << 32) * 3 * 5 * 17 * 257 * 65537)


@pytest.mark.parametrize("field", FIELDS)
def test_permutation_round_structure(field):
    """the rounds written out once more, with pow and the explicit matrices"""
    p, t = M.MODULUS[field], M.WIDTH[field]
    me = circ_external(t)
    rng = np.random.default_rng(3)
    for rf, rp in ROUNDS[field]:
        prm = params(field, rf, rp, seed=rf + rp)
        m = M.of_params(prm)
        assert len(m.ce) == rf and len(m.ci) == rp and len(m.d) == t and all(m.d)
        mi = [[(m.d[i] if i == j else 0) + 1 for j in range(t)] for i in range(t)]
        x0 = rand_state(field, rng)
        x = matvec(me, x0, p)
        for r in range(rf // 2):
            x = matvec(me, [pow(x[i] + m.ce[r][i], 7, p) for i in range(t)], p)
        for r in range(rp):
            x[0] = pow(x[0] + m.ci[r], 7, p)
            x = matvec(mi, x, p)
        for r in range(rf // 2, rf):
            x = matvec(me, [pow(x[i] + m.ce[r][i], 7, p) for i in range(t)], p)
        assert M.permute(x0, m) == x
        from sppark_amd import poseidon2
        assert poseidon2.permute_ints(x0, prm) == x                                      # the package's verifier agrees


@pytest.mark.parametrize("field", FIELDS)
def test_batch_form_equals_one_state_form(field):
    rng = np.random.default_rng(4)
    m = M.of_params(params(field, *M.USUAL[field]))
    states = rand_state(field, rng, 9)
    states[0, :] = 0
    states[1, :] = M.MODULUS[field] - 1
    got = M.permute([states[:, i] for i in range(m.t)], m)
    for k in range(len(states)):
        assert [int(got[i][k]) for i in range(m.t)] == M.permute([int(v) for v in states[k]], m)


@pytest.mark.parametrize("field", FIELDS)
def test_sponge_permutation_counts_and_overwrite(field):
    m = M.of_params(params(field, *M.USUAL[field]))
    rate, t, p = m.rate, m.t, m.p
    rng = np.random.default_rng(5)
    for width, want in ((1, 1), (rate - 1, 1), (rate, 1), (rate + 1, 2), (2 * rate - 1, 2), (2 * rate, 2), (2 * rate + 1, 3), (3 * rate - 1, 3),
                        (3 * rate, 3)):
        leaf = [int(v) % p for v in rng.integers(1, 1 << 62, width)]
        before = M.PERMUTATIONS[0]
        got = M.leaf_digest(leaf, m)
        assert M.PERMUTATIONS[0] - before == want == -(-width // rate), width
        # by hand: overwrite, permute, overwrite only the positions of a partial chunk
        x = [0] * t
        for at in range(0, width, rate):
            for k, v in enumerate(leaf[at:at + rate]):
                x[k] = v
            x = M.permute(x, m)
        assert got == x[:m.out] and len(got) == t // 2
    # no padding: a leaf of RATE elements is one permutation of (leaf || 0); a trailing zero element is NOT the same leaf
    leaf = [int(v) % p for v in rng.integers(1, 1 << 62, rate)]
    assert M.leaf_digest(leaf, m) == M.permute(leaf + [0] * rate, m)[:m.out]
    assert M.leaf_digest(leaf + [0], m) != M.leaf_digest(leaf, m)
    # a partial last chunk leaves the capacity AND the rest of the rate as the permutation left them
    two = leaf + [7]
    x = M.permute(leaf + [0] * rate, m)
    x[0] = 7
    assert M.leaf_digest(two, m) == M.permute(x, m)[:m.out]
    # node: no feed-forward, left before right
    a, b = M.leaf_digest(leaf, m), M.leaf_digest(two, m)
    assert M.node(a, b, m) == M.permute(a + b, m)[:m.out] != M.node(b, a, m)


@pytest.mark.parametrize("field", FIELDS)
def test_wire_format_round_trip(field):
    p = M.MODULUS[field]
    from sppark_amd import poseidon2
    vals = [0, 1, 2, p - 1, 12345678]
    wire = [int(M.to_wire(field, v)) for v in vals]
    assert wire == poseidon2.to_wire(field, vals) and poseidon2.from_wire(field, wire) == vals
    assert wire[1] == (0x0ffffffe if field == "bb31" else 1)                             # Montgomery one, R = 2^32
    assert [int(v) for v in M.values(field, np.array(wire, dtype=M.wire_dtype(field)))] == vals
    assert M.wire_bytes(field, vals) == np.array(wire, dtype=M.wire_dtype(field)).tobytes()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("lg", (0, 1, 3, 5))
def test_verify_accepts_the_honest_path_only(field, lg):
    from sppark_amd import poseidon2
    prm = params(field, 8, 1)
    m = M.of_params(prm)
    width, n = m.rate + 1, 1 << lg
    rng = np.random.default_rng(6 + lg)
    leaves = np.array([[int(v) % m.p for v in rng.integers(0, 1 << 62, width)] for _ in range(n)], dtype=M.value_dtype(field))
    lay = M.layers(leaves, m)
    assert [x.shape for x in lay] == [(n >> l, m.out) for l in range(lg + 1)]
    root = M.digest_bytes(field, lay, lg, 0)
    assert M.tree_bytes(field, lay)[-32:].tobytes() == root
    for index in sorted({0, n - 1, n // 2, n // 3}):
        leaf_wire = np.frombuffer(M.wire_bytes(field, leaves[index]), dtype=M.wire_dtype(field))
        path = M.path(field, lay, index)
        assert len(path) == lg
        assert poseidon2.verify(root, index, leaf_wire, path, prm)
        assert poseidon2.verify(np.frombuffer(root, dtype=np.uint8), index, leaf_wire.tobytes(), [np.frombuffer(q, dtype=np.uint8) for q in path], prm)
        assert M.verify(m, root, index, [int(v) for v in leaves[index]], path)
        flipped = leaf_wire.copy()
        flipped[width - 1] ^= 1
        assert not poseidon2.verify(root, index, flipped, path, prm)
        bad_root = bytearray(root)
        bad_root[31] ^= 0x01
        assert not poseidon2.verify(bytes(bad_root), index, leaf_wire, path, prm)
        assert not poseidon2.verify(root, index + n, leaf_wire, path, prm) and not poseidon2.verify(root, -1, leaf_wire, path, prm)
        assert not poseidon2.verify(root, index, leaf_wire[:-1], path, prm)
        if lg:
            assert not poseidon2.verify(root, index ^ 1, leaf_wire, path, prm)           # a wrong index
            bit = bytearray(path[lg - 1])
            bit[0] ^= 0x80 if field == "gl64" else 0x01
            assert not poseidon2.verify(root, index, leaf_wire, path[:-1] + [bytes(bit)], prm)
            assert not poseidon2.verify(root, index, leaf_wire, path[:-1], prm)
        if lg >= 2:
            swapped = [path[1], path[0]] + path[2:]
            assert not poseidon2.verify(root, index, leaf_wire, swapped, prm)            # swapped siblings


def test_test_params_are_reproducible_canonical_and_distinct():
    from sppark_amd import poseidon2
    for field in FIELDS + ("bb31_canonical", "gl64_plonky2"):
        t, p = M.WIDTH[field], M.MODULUS[field]
        a, b, c = poseidon2.test_params(field), poseidon2.test_params(field), poseidon2.test_params(field, seed=1)
        assert (a.rounds_f, a.rounds_p) == M.USUAL[field] and len(a.consts) == 8 * t + a.rounds_p + t
        assert (a.consts == b.consts).all() and (a.consts != c.consts).any()
        assert int(a.consts.max()) < p and a.consts.dtype == M.wire_dtype(field) and (a.consts[-t:] != 0).all()
        assert len(set(a.consts.tolist())) > len(a.consts) - 2
    with pytest.raises(ValueError):
        poseidon2.test_params("m31")
