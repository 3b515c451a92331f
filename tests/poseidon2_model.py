"""Host model of Poseidon2 as include/sppark_amd_poseidon2.h defines it: the permutation, the overwrite sponge, the tree.

Everything is computed on CANONICAL integers modulo p.  A "value" is a Python integer or a numpy array of them (one entry per
state of a batch): uint64 for BabyBear, where every intermediate stays below 2^62, dtype=object (Python integers) for
Goldilocks.  The same few lines serve one state and a batch of them, because they use only +, * and % p.  Wire format
(to_wire / from_wire): Montgomery words with R = 2^32 for bb31, the canonical integer itself for gl64."""
import numpy as np

MODULUS = {"bb31": 0x78000001, "bb31_canonical": 0x78000001, "gl64": 0xffffffff00000001, "gl64_plonky2": 0xffffffff00000001}
WIDTH = {"bb31": 16, "bb31_canonical": 16, "gl64": 8, "gl64_plonky2": 8}
MONT_BITS = {"bb31": 32, "bb31_canonical": 32, "gl64": 0, "gl64_plonky2": 0}
USUAL = {"bb31": (8, 13), "bb31_canonical": (8, 13), "gl64": (8, 22), "gl64_plonky2": (8, 22)}
M4 = ((2, 3, 1, 1), (1, 2, 3, 1), (1, 1, 2, 3), (3, 1, 1, 2))
DIGEST = 32
PERMUTATIONS = [0]                                          # calls of permute(), for the tests that count them


def wire_dtype(field):
    return np.uint32 if WIDTH[field] == 16 else np.uint64


def value_dtype(field):
    return np.uint64 if WIDTH[field] == 16 else object


def to_wire(field, v):
    """canonical -> wire; an integer or an array of value_dtype"""
    p, k = MODULUS[field], MONT_BITS[field]
    return (v << k) % p if k else v


def from_wire(field, w):
    p, k = MODULUS[field], MONT_BITS[field]
    return (w * pow(1 << k, -1, p)) % p if k else w


def values(field, words):
    """an array of wire words (any integer dtype) -> an array of canonical values of value_dtype"""
    return from_wire(field, np.asarray(words).astype(value_dtype(field)))


def wire_bytes(field, vals):
    """a sequence of canonical values (Python integers) -> their wire bytes"""
    return np.array([int(to_wire(field, int(v))) for v in vals], dtype=wire_dtype(field)).tobytes()


class Model:
    """one parameter set on canonical integers: ce[r][i], ci[r], d[i]"""

    def __init__(self, field, rounds_f, rounds_p, wire_consts):
        self.field, self.p, self.t = field, MODULUS[field], WIDTH[field]
        self.rate = self.out = self.t // 2
        self.rounds_f, self.rounds_p = rounds_f, rounds_p
        c = [int(from_wire(field, int(w))) for w in np.asarray(wire_consts).reshape(-1).tolist()]
        t = self.t
        assert len(c) == rounds_f * t + rounds_p + t and rounds_f % 2 == 0
        self.ce = [c[r * t:(r + 1) * t] for r in range(rounds_f)]
        self.ci = c[rounds_f * t:rounds_f * t + rounds_p]
        self.d = c[rounds_f * t + rounds_p:]


def of_params(params):
    """the model of a sppark_amd.poseidon2.Params"""
    return Model(params.field, params.rounds_f, params.rounds_p, params.consts)


def sbox(x, p):
    x2 = (x * x) % p
    x3 = (x2 * x) % p
    x4 = (x2 * x2) % p
    return (x3 * x4) % p


def external(x, p):
    """M_E: z_b = M4 x_b, s = sum_b z_b, y_b = z_b + s"""
    z = []
    for b in range(0, len(x), 4):
        for row in M4:
            z.append((row[0] * x[b] + row[1] * x[b + 1] + row[2] * x[b + 2] + row[3] * x[b + 3]) % p)
    s = []
    for k in range(4):
        acc = z[k]
        for b in range(4, len(x), 4):
            acc = (acc + z[b + k]) % p
        s.append(acc)
    return [(z[i] + s[i % 4]) % p for i in range(len(x))]


def internal(x, d, p):
    """M_I: s = sum_i x_i, y_i = d_i x_i + s"""
    s = x[0]
    for v in x[1:]:
        s = (s + v) % p
    return [((d[i] * x[i]) % p + s) % p for i in range(len(x))]


def permute(x, m):
    """the permutation of a state: a list of T values"""
    PERMUTATIONS[0] += 1
    p, half = m.p, m.rounds_f // 2
    assert len(x) == m.t
    x = external(list(x), p)
    for r in range(half):
        x = external([sbox((x[i] + m.ce[r][i]) % p, p) for i in range(m.t)], p)
    for r in range(m.rounds_p):
        x[0] = sbox((x[0] + m.ci[r]) % p, p)
        x = internal(x, m.d, p)
    for r in range(half, m.rounds_f):
        x = external([sbox((x[i] + m.ce[r][i]) % p, p) for i in range(m.t)], p)
    return x


def leaf_digest(elems, m):
    """the overwrite sponge over a leaf: a list of width values -> OUT values"""
    zero = elems[0] * 0                                                                  # (an integer or an array of zeros)
    x = [zero] * m.t
    for at in range(0, len(elems), m.rate):
        chunk = elems[at:at + m.rate]
        x[:len(chunk)] = chunk
        x = permute(x, m)
    return x[:m.out]


def node(left, right, m):
    return permute(list(left) + list(right), m)[:m.out]


# ---- whole trees, vectorised over the leaves ---------------------------------------------------------------------------------
def layers(leaves, m):
    """leaves: an array (n, width) of canonical values (value_dtype) -> [layer 0 .. layer lg_n], layer l an array (n >> l, OUT)"""
    n = leaves.shape[0]
    assert n and n & (n - 1) == 0
    cur = leaf_digest([leaves[:, j] for j in range(leaves.shape[1])], m)
    out = [np.stack(cur, axis=1)]
    while out[-1].shape[0] > 1:
        prev = out[-1]
        cur = node([prev[0::2, k] for k in range(m.out)], [prev[1::2, k] for k in range(m.out)], m)
        out.append(np.stack(cur, axis=1))
    return out


def layer_bytes(field, layer):
    """a layer (m, OUT) of canonical values -> its wire bytes"""
    flat = to_wire(field, layer.reshape(-1))
    return np.array(flat.tolist(), dtype=wire_dtype(field)).tobytes()


def tree_bytes(field, lay):
    """the layers as the entry point stores them: bottom-up, the root last; a uint8 array"""
    return np.frombuffer(b"".join(layer_bytes(field, x) for x in lay), dtype=np.uint8).copy()


def digest_bytes(field, lay, l, i):
    return layer_bytes(field, lay[l][i:i + 1])


def path(field, lay, index):
    """the siblings on the way up from leaf |index|, as 32-byte strings"""
    return [digest_bytes(field, lay, l, (index >> l) ^ 1) for l in range(len(lay) - 1)]


def leaves_of(field, words, n, width, col_stride, leaf_stride):
    """the (n, width) canonical leaves of a flat array of wire words that holds a matrix with the given strides (in elements)"""
    flat = np.asarray(words).reshape(-1)
    idx = (np.arange(width)[None, :] * col_stride + np.arange(n)[:, None] * leaf_stride)
    return values(field, flat[idx])


# ---- large trees without a large model (tests/merkle_model.py has the byte-hash versions) ---------------------------------------
def zero_digests(m, width, lg_n):
    """Z_0 = the digest of a leaf of zeros, Z_l = node(Z_{l-1}, Z_{l-1}), as lists of integers"""
    z = [leaf_digest([0] * width, m)]
    for _ in range(lg_n):
        z.append(node(z[-1], z[-1], m))
    return z


def planted(m, width, lg_n, plants):
    """The tree over a matrix that is zero except for the leaves in |plants| ({index: list of canonical elements}): per layer a
    dict {position: digest bytes} of the digests that differ from Z_l, the Z_l as bytes, and the root's bytes."""
    z = zero_digests(m, width, lg_n)
    cur = {i: leaf_digest([int(v) for v in leaf], m) for i, leaf in plants.items()}
    sparse = [dict(cur)]
    for l in range(lg_n):
        nxt = {}
        for i in cur:
            q = i >> 1
            if q not in nxt:
                nxt[q] = node(cur.get(2 * q, z[l]), cur.get(2 * q + 1, z[l]), m)
        cur = nxt
        sparse.append(dict(cur))
    root = cur.get(0, z[lg_n])
    as_bytes = lambda dg: wire_bytes(m.field, dg)                                        # noqa: E731
    return [{i: as_bytes(dg) for i, dg in layer.items()} for layer in sparse], [as_bytes(x) for x in z], as_bytes(root)


def periodic(m, pool_leaves, lg_n):
    """The tree over 2^lg_n leaves that repeat |pool_leaves| ((2^k, width) canonical values): (the pool's layers, the wire
    bytes of the one digest of layers k, k + 1, .., lg_n)."""
    lay = layers(pool_leaves, m)
    k = len(lay) - 1
    x = [int(v) for v in lay[k][0]]
    above = [wire_bytes(m.field, x)]
    for _ in range(lg_n - k):
        x = node(x, x, m)
        above.append(wire_bytes(m.field, x))
    return lay, above


def verify(m, root, index, leaf, siblings):
    """leaf: canonical elements; root and siblings: 32 wire bytes each"""
    as_ints = lambda b: [int(v) for v in values(m.field, np.frombuffer(bytes(b), dtype=wire_dtype(m.field)))]   # noqa: E731
    x = leaf_digest([int(v) for v in leaf], m)
    if index < 0 or index >> len(siblings):
        return False
    for l, sib in enumerate(siblings):
        x = node(as_ints(sib), x, m) if (index >> l) & 1 else node(x, as_ints(sib), m)
    return wire_bytes(m.field, x) == bytes(root)
