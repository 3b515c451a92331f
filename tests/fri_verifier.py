"""A FRI / DEEP verifier on Python integers, written from the mathematical definition and the text of
include/sppark_amd_fri.h -- neither from tests/fri_model.py nor from the kernels.  It sees what a verifier sees: roots, the
claimed openings, opened leaves with their authentication paths and the final layer.  If it accepts a transcript that a
prover made with the library's calls, those calls compose into a prover; if a convention between two of them is off (the
coset or order a transform leaves, which elements make a fold group and which leaf holds them, the shift of a folded
domain, a base-field trace under extension-field challenges) it rejects.

Host only.  It uses hashlib, sppark_amd.merkle.verify (pure hashlib), mle_model.Model for field arithmetic and wire-form
conversion, and from the oracle only the root of unity of order 2^lg and the coset generator.  Inverses are base-field
inverses, pow(x, -1, p): the points of a domain are base-field elements.

The transcript is a plain dict; the prover fills it, the verifier reads it:
    trace_field, field    the field of the trace matrices and of the codeword (the same, or "bb31" under "bb31x4")
    hash                  "blake2s" or "sha256": the hash of every tree (challenges always come from blake2s)
    order                 NATURAL or BITREV: index i of a vector holds x_i = shift * w^i or shift * w^bitrev(i)
    lg_n, lg_blowup       the first codeword has 2^lg_n elements; the trace polynomials have 2^(lg_n - lg_blowup) coefficients
    arities               a_0 .. a_{L-1}: layer r is folded 2^a_r to one
    widths                columns of each trace matrix
    forced                query indices that are asked for whatever the transcript says, before the drawn ones
    trace_roots           one root per trace matrix
    z, openings           the out-of-domain point and the claimed f_j(z), wire bytes of |field|
    layer_roots           the root of every FRI layer 0 .. L-1; the leaf of layer r is one fold group of 2^a_r elements
    final                 the codeword after the last fold, in full, wire bytes
    queries               per query index, in the order indices() gives them:
                          {"trace": [(leaf bytes, path)] per matrix, "layers": [(leaf bytes, path)] per layer}

Challenges come from hashlib.blake2s over the transcript so far (FiatShamir below, which prover and verifier share); the
verifier recomputes all of them and takes none from the prover -- except when verify() is handed |challenges|, for a prover
that had to draw them before it ran.

verify() returns None or the name of the first failed check:
    "shape"       the transcript's parameters or sizes make no sense
    "z"           z is not the point the transcript implies, or lies inside a domain
for every query in turn
    "trace_path"  an opened trace leaf does not verify at the query's index
    "layer_path"  an opened fold group does not verify at the leaf index the query's index implies
    "deep"        q (x_i - z) != sum_j alpha^j f_j(x_i) - sum_j alpha^j v_j
    "fold"        the next layer's value at the group's index (after the last fold: the final layer's entry) is not the fold
                  of the group
and at the end
    "final"       the final layer is not of the degree the schedule leaves"""
import hashlib

import numpy as np

from mle_model import Model

NATURAL, BITREV = 0, 1
BASE_OF = {"bb31x4": "bb31"}
DRAWN_QUERIES = 12
MAX_FINAL = 32


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def root_of_unity(base_field, lg):
    """the oracle's root of order 2^lg: its transform of X over 2^lg points holds w^i at index i"""
    from fri_model import _oracle_x
    return _oracle_x(base_field, lg, False)[1] if lg else 1


def coset_generator(base_field):
    """the oracle's coset generator: its Coset transform of X starts with g"""
    from fri_model import _oracle_x
    return _oracle_x(base_field, 1, True)[0]


def point(shift, w, lg, order, i, p):
    """the header's formula: NATURAL x_i = shift * w^i, BITREV x_i = shift * w^bitrev_lg(i)"""
    return shift * pow(w, bitrev(i, lg) if order == BITREV else i, p) % p


def to_bytes(m, vals):
    return np.ascontiguousarray(m.rows(list(vals))).tobytes()


def from_bytes(m, data):
    f = m.f
    if len(data) % (f.w * np.dtype(f.dtype).itemsize):
        raise ValueError("not a whole number of elements")
    return m.vals(np.frombuffer(bytes(data), dtype=f.dtype).reshape(-1, f.w))


def elem_bytes(m):
    return m.f.w * np.dtype(m.f.dtype).itemsize


def embed(m, x):
    return (x % m.p, 0, 0, 0) if m.x4 else x % m.p


def outside(m, z, g, lg_n, lg_blowup):
    """z lies neither on the evaluation domain g * <w_n> nor on the trace domain <w_(n / blow-up)>"""
    if m.x4:
        if any(z[1:]):
            return True
        z = z[0]
    if z == 0:
        return True
    p = m.p
    return pow(z * pow(g, -1, p) % p, 1 << lg_n, p) != 1 and pow(z, 1 << (lg_n - lg_blowup), p) != 1


class FiatShamir:
    """The challenges of a transcript: a blake2s chain over what the transcript holds so far.  Each method absorbs what the
    prover has put into the dict since the last one and must be called in this order: z, alpha, beta(0) .., indices."""
    def __init__(self, t):
        self.t, self.m = t, Model(t["field"])
        head = repr((t["trace_field"], t["field"], t["hash"], int(t["order"]), int(t["lg_n"]), int(t["lg_blowup"]),
                     tuple(int(a) for a in t["arities"]), tuple(int(w) for w in t["widths"]), tuple(int(i) for i in t["forced"])))
        self.state = hashlib.blake2s(head.encode()).digest()
        self.count = 0
        self.z_draws = 0

    def absorb(self, *chunks):
        for c in chunks:
            self.state = hashlib.blake2s(self.state + bytes(c)).digest()

    def integer(self, modulus):
        """64 bytes of the chain, reduced"""
        out = b""
        for _ in range(2):
            out += hashlib.blake2s(self.state + self.count.to_bytes(8, "little")).digest()
            self.count += 1
        return int.from_bytes(out, "little") % modulus

    def element(self):
        """one draw per component"""
        p = self.m.p
        return tuple(self.integer(p) for _ in range(4)) if self.m.x4 else self.integer(p)

    def z(self):
        t = self.t
        self.absorb(*t["trace_roots"])
        g = coset_generator(BASE_OF.get(t["field"], t["field"]))
        while True:
            z = self.element()
            self.z_draws += 1
            if outside(self.m, z, g, t["lg_n"], t["lg_blowup"]):
                return z

    def alpha(self):
        self.absorb(self.t["z"], *self.t["openings"])
        return self.element()

    def beta(self, r):
        self.absorb(self.t["layer_roots"][r])
        return self.element()

    def indices(self):
        self.absorb(self.t["final"])
        n = 1 << self.t["lg_n"]
        return [int(i) for i in self.t["forced"]] + [self.integer(n) for _ in range(DRAWN_QUERIES)]


def group_of(order, lg, a, i):
    """(leaf index of the fold group that holds index i of a layer of 2^lg elements, i's position in that leaf): the header's
    "a lane holds the 2^a inputs of a group: contiguous in BITREV, n / 2^a apart in NATURAL" """
    if order == BITREV:
        return i >> a, i & ((1 << a) - 1)
    return i & ((1 << (lg - a)) - 1), i >> (lg - a)


def member_index(order, lg, a, j, pos):
    """the inverse of group_of"""
    return (j << a) + pos if order == BITREV else j + (pos << (lg - a))


def final_check(m, final, d, w, order, lg):
    """is the final codeword, 2^lg values on a coset of <w>, a polynomial of degree below d?  d == 1: all entries are equal.
    Otherwise the inverse DFT: c_k = shift^-k / n * sum_i f_i w^(-ik), and only whether c_k is zero is asked, so the
    non-zero factor shift^-k / n is left out."""
    n = 1 << lg
    if d == 1:
        return all(v == final[0] for v in final)
    nat = [final[bitrev(i, lg)] for i in range(n)] if order == BITREV else list(final)
    winv = pow(w, -1, m.p)
    for k in range(d, n):
        s = m.zero
        for i, v in enumerate(nat):
            s = m.add(s, m.smul(pow(winv, i * k, m.p), v))
        if s != m.zero:
            return False
    return True


def verify(t, challenges=None):
    """None, or the name of the first failed check.  challenges: None, or {"z", "alpha", "betas", "indices"} as values"""
    try:
        return _verify(t, challenges)
    except (KeyError, IndexError, ValueError, TypeError):
        return "shape"


def _verify(t, challenges):
    from sppark_amd import merkle
    field, trace_field, hash_, order = t["field"], t["trace_field"], t["hash"], t["order"]
    m, tm = Model(field), Model(trace_field)
    base = BASE_OF.get(field, field)
    p = m.p
    lg_n, lg_blowup, arities, widths = int(t["lg_n"]), int(t["lg_blowup"]), [int(a) for a in t["arities"]], [int(w) for w in t["widths"]]
    k = lg_n - lg_blowup
    lifted = trace_field != field
    if (order not in (NATURAL, BITREV) or k < 0 or not arities or any(not 1 <= a <= 3 for a in arities) or sum(arities) > k
            or (lifted and BASE_OF.get(field) != trace_field) or len(t["trace_roots"]) != len(widths)
            or len(t["layer_roots"]) != len(arities) or len(t["openings"]) != sum(widths)):
        return "shape"
    w, g = root_of_unity(base, lg_n), coset_generator(base)
    assert pow(w, 1 << lg_n, p) == 1 and (lg_n == 0 or pow(w, 1 << (lg_n - 1), p) == p - 1)

    # ---- challenges ----
    if challenges is None:
        fs = FiatShamir(t)
        z = fs.z()
        if to_bytes(m, [z]) != bytes(t["z"]):
            return "z"
        alpha = fs.alpha()
        betas = [fs.beta(r) for r in range(len(arities))]
        indices = fs.indices()
    else:
        z, alpha, betas, indices = challenges["z"], challenges["alpha"], list(challenges["betas"]), [int(i) for i in challenges["indices"]]
        if to_bytes(m, [z]) != bytes(t["z"]) or not outside(m, z, g, lg_n, lg_blowup):
            return "z"
    if len(betas) != len(arities) or len(t["queries"]) != len(indices) or any(not 0 <= i < 1 << lg_n for i in indices):
        return "shape"
    v = from_bytes(m, b"".join(bytes(x) for x in t["openings"]))
    if len(v) != sum(widths):
        return "shape"

    total = sum(arities)
    lg_final = lg_n - total
    final = from_bytes(m, t["final"])
    if len(final) != 1 << lg_final or len(final) > MAX_FINAL:
        return "shape"

    apow = [m.one]
    for _ in range(len(v) - 1):
        apow.append(m.mul(apow[-1], alpha))
    claimed = m.zero                                                    # sum_j alpha^j v_j
    for a_j, v_j in zip(apow, v):
        claimed = m.add(claimed, m.mul(a_j, v_j))

    for i, q in zip(indices, t["queries"]):
        # ---- 1. every opened leaf, at the index the verifier derives ----
        f_x = []                                                        # f_j(x_i), values of the trace field
        if len(q["trace"]) != len(widths) or len(q["layers"]) != len(arities):
            return "shape"
        for (leaf, path), root, width in zip(q["trace"], t["trace_roots"], widths):
            if len(leaf) != width * elem_bytes(tm) or len(path) != lg_n or not merkle.verify(root, i, leaf, path, hash=hash_):
                return "trace_path"
            f_x += from_bytes(tm, leaf)
        groups = []                                                     # per layer: (leaf index, position of the followed index, members)
        at, lg = i, lg_n
        for r, a in enumerate(arities):
            j, pos = group_of(order, lg, a, at)
            leaf, path = q["layers"][r]
            if (len(leaf) != elem_bytes(m) << a or len(path) != lg - a
                    or not merkle.verify(t["layer_roots"][r], j, leaf, path, hash=hash_)):
                return "layer_path"
            groups.append((j, pos, from_bytes(m, leaf)))
            at, lg = j, lg - a

        # ---- 2. DEEP ----
        x_i = point(g, w, lg_n, order, i, p)
        quotient = groups[0][2][groups[0][1]]
        combined = m.zero
        for a_j, f_j in zip(apow, f_x):
            combined = m.add(combined, m.smul(f_j, a_j) if lifted else m.mul(a_j, f_j))
        if m.mul(quotient, m.sub(embed(m, x_i), z)) != m.sub(combined, claimed):
            return "deep"

        # ---- 3. and 4. the folds ----
        shift, w_r, lg = g, w, lg_n
        for r, a in enumerate(arities):
            A = 1 << a
            j, _pos, members = groups[r]
            zeta = pow(w_r, 1 << (lg - a), p)                           # of order A
            x = point(shift, w_r, lg, order, member_index(order, lg, a, j, 0), p)
            by_t = [None] * A                                           # f(x zeta^t)
            for pos in range(A):
                tt = bitrev(pos, a) if order == BITREV else pos
                # each member's point from its own index, by the header's formula
                assert point(shift, w_r, lg, order, member_index(order, lg, a, j, pos), p) == x * pow(zeta, tt, p) % p
                by_t[tt] = members[pos]
            c = m.smul(pow(x, -1, p), betas[r])                         # beta / x
            acc, ck = m.zero, m.one
            for kk in range(A):
                inner = m.zero
                for tt in range(A):
                    inner = m.add(inner, m.smul(pow(zeta, -tt * kk, p), by_t[tt]))
                acc = m.add(acc, m.mul(ck, inner))
                ck = m.mul(ck, c)
            folded = m.smul(pow(A, -1, p), acc)
            if r + 1 < len(arities):
                target = groups[r + 1][2][groups[r + 1][1]]
            else:
                target = final[j]
            if folded != target:
                return "fold"
            shift, w_r, lg = pow(shift, A, p), pow(w_r, A, p), lg - a
            assert point(shift, w_r, lg, order, j, p) == pow(x, A, p)   # the folded value sits over x^A
    # ---- 5. the final layer ----
    if not final_check(m, final, 1 << (k - total), pow(w, 1 << total, p), order, lg_final):
        return "final"
    return None
