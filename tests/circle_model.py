"""Host model of the circle transform over Mersenne31 (include/sppark_amd_circle.h), written from the
definition and independent of the kernels: pure Python for the definition itself, uint64 numpy for the
fast network.

  group      C = {(x, y): x^2 + y^2 = 1},  (x0, y0)(x1, y1) = (x0 x1 - y0 y1, x0 y1 + y0 x1)
  generator  G = (2, 1268011823) of order 2^31;  g_m = G^(2^(31 - m)) has order 2^m
  domain     D_k: H_i = g_{k+1}^(4i + 1), i < n/2;  D_i = H_i, D_{i + n/2} = conj(H_i)
  basis      b_j = y^j0 x^j1 pi(x)^j2 pi^2(x)^j3 ...,  pi(x) = 2x^2 - 1
  forward    e_i = sum_j c_j b_j(D_i);  BITREV (0): position q holds e_{bitrev_k(q)};  NATURAL (1): position i holds e_i
"""
import numpy as np

P = (1 << 31) - 1
G = (2, 1268011823)
BITREV, NATURAL = 0, 1
FORWARD, INVERSE = 0, 1
MAX_LG = 30


def cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def gpow(e):
    """G^e for a Python integer e >= 0."""
    r, b = (1, 0), G
    while e:
        if e & 1:
            r = cmul(r, b)
        b = cmul(b, b)
        e >>= 1
    return r


def g_of_order(m):
    return gpow(1 << (31 - m))


def bitrev(x, bits):
    r = 0
    for i in range(bits):
        r |= ((x >> i) & 1) << (bits - 1 - i)
    return r


def bitrev_perm(k):
    """numpy index array q -> bitrev_k(q)."""
    idx = np.arange(1 << k, dtype=np.uint64)
    r = np.zeros_like(idx)
    for i in range(k):
        r |= ((idx >> np.uint64(i)) & np.uint64(1)) << np.uint64(k - 1 - i)
    return r.astype(np.int64)


# ---- G^e for arrays of exponents: three small tables of points, two group products ----
_T = None


def _tables():
    global _T
    if _T is None:
        def tab(count, step):
            out = np.zeros((count, 2), dtype=np.uint64)
            s, cur = gpow(step), (1, 0)
            for i in range(count):
                out[i] = cur
                cur = cmul(cur, s)
            return out
        _T = (tab(1 << 10, 1), tab(1 << 11, 1 << 10), tab(1 << 10, 1 << 21))
    return _T


def _vmul(a, b):
    ax, ay, bx, by = a[..., 0], a[..., 1], b[..., 0], b[..., 1]
    x = (ax * bx % P + (P - ay * by % P)) % P
    y = (ax * by % P + ay * bx % P) % P
    return np.stack([x, y], axis=-1)


def gpow_vec(e):
    """(len(e), 2) uint64 points G^e for a numpy array of exponents < 2^31."""
    e = np.asarray(e, dtype=np.uint64)
    t0, t1, t2 = _tables()
    return _vmul(_vmul(t2[(e >> np.uint64(21)).astype(np.int64)], t1[((e >> np.uint64(10)) & np.uint64(0x7ff)).astype(np.int64)]),
                 t0[(e & np.uint64(0x3ff)).astype(np.int64)])


def domain_points(k, idx):
    """The points D_i of D_k for an array of domain indices i, (len, 2) uint64."""
    idx = np.asarray(idx, dtype=np.uint64)
    n = 1 << k
    if k == 0:
        return np.tile(np.array([[1, 0]], dtype=np.uint64), (len(idx), 1))
    half = np.uint64(n // 2)
    lo = idx % half if n > 1 else idx
    pts = gpow_vec((np.uint64(4) * lo + np.uint64(1)) << np.uint64(30 - k))
    conj = idx >= half
    pts[conj, 1] = (P - pts[conj, 1]) % P
    return pts


def domain(k, evals_order=NATURAL):
    """(2^k, 2) uint32 array of the points of D_k in the given evaluation order."""
    idx = np.arange(1 << k, dtype=np.int64)
    if evals_order == BITREV:
        idx = bitrev_perm(k)
    return domain_points(k, idx).astype(np.uint32)


def domain_direct(k):
    """D_k straight from the definition, Python integers."""
    n = 1 << k
    if k == 0:
        return [(1, 0)]
    g = g_of_order(k + 1)
    g4, cur, h = cmul(cmul(g, g), cmul(g, g)), g, []
    for _ in range(n // 2):
        h.append(cur)
        cur = cmul(cur, g4)
    return h + [(x, (P - y) % P) for (x, y) in h]


def basis_direct(j, k, pt):
    x, y = pt
    v = 1
    if j & 1:
        v = y
    t = x
    for bit in range(1, k):
        if (j >> bit) & 1:
            v = v * t % P
        t = (2 * t * t - 1) % P
    return v


def direct_evaluate(c, k):
    """Natural-order evaluations from the definition, O(n^2)."""
    d = domain_direct(k)
    return [sum(int(c[j]) * basis_direct(j, k, pt) for j in range(1 << k)) % P for pt in d]


# ---- the in-place network, vectorised ----
def _x_twiddles(k, b):
    """Twiddles of x-layer b (1 <= b <= k - 1) for the blocks h < 2^(k-1-b)."""
    bits = k - 1 - b
    h = bitrev_perm(bits).astype(np.uint64)
    e = ((np.uint64(4) * h + np.uint64(1)) << np.uint64(b - 1)) << np.uint64(30 - k)
    return gpow_vec(e)[:, 0]


def _y_twiddles(k):
    h = bitrev_perm(k - 1).astype(np.uint64)
    return gpow_vec((np.uint64(4) * h + np.uint64(1)) << np.uint64(30 - k))[:, 1]


def _inv(a):
    a = np.asarray(a, dtype=np.uint64)
    r = np.ones_like(a)
    e, b = P - 2, a.copy()
    while e:
        if e & 1:
            r = r * b % P
        b = b * b % P
        e >>= 1
    return r


def forward(c, k, evals_order=BITREV):
    """Evaluate: coefficients (natural index order) along the last axis -> evaluations."""
    a = np.array(c, dtype=np.uint64)
    shape, n = a.shape, 1 << k
    assert shape[-1] == n
    a = a.reshape(-1, n)
    for b in range(k - 1, 0, -1):
        t = _x_twiddles(k, b)
        v = a.reshape(a.shape[0], -1, 2, 1 << b)
        u, w = v[:, :, 0, :].copy(), v[:, :, 1, :] * t[None, :, None] % P
        v[:, :, 0, :] = (u + w) % P
        v[:, :, 1, :] = (u + P - w) % P
    if k >= 1:
        t = _y_twiddles(k)
        v = a.reshape(a.shape[0], -1, 2)
        u, w = v[:, :, 0].copy(), v[:, :, 1] * t[None, :] % P
        v[:, :, 0] = (u + w) % P
        v[:, :, 1] = (u + P - w) % P
    if evals_order == NATURAL:
        out = np.empty_like(a)
        out[:, bitrev_perm(k)] = a
        a = out
    return a.reshape(shape).astype(np.uint32)


def inverse(e, k, evals_order=BITREV):
    """Interpolate: evaluations -> coefficients, the 1/n included."""
    a = np.array(e, dtype=np.uint64)
    shape, n = a.shape, 1 << k
    assert shape[-1] == n
    a = a.reshape(-1, n)
    if evals_order == NATURAL:
        a = a[:, bitrev_perm(k)].copy()
    if k >= 1:
        t = _inv(_y_twiddles(k))
        v = a.reshape(a.shape[0], -1, 2)
        u, w = v[:, :, 0].copy(), v[:, :, 1].copy()
        v[:, :, 0] = (u + w) % P
        v[:, :, 1] = (u + P - w) % P * t[None, :] % P
    for b in range(1, k):
        t = _inv(_x_twiddles(k, b))
        v = a.reshape(a.shape[0], -1, 2, 1 << b)
        u, w = v[:, :, 0, :].copy(), v[:, :, 1, :].copy()
        v[:, :, 0, :] = (u + w) % P
        v[:, :, 1, :] = (u + P - w) % P * t[None, :, None] % P
    a = a * np.uint64(pow(n, P - 2, P)) % P
    return a.reshape(shape).astype(np.uint32)


def lde(e, k, blowup, evals_order=BITREV):
    """Evaluations on D_k -> (coefficients, evaluations on D_{k+blowup}), same order in and out."""
    coeffs = inverse(e, k, evals_order)
    pad = np.zeros(coeffs.shape[:-1] + (1 << (k + blowup),), dtype=np.uint32)
    pad[..., :1 << k] = coeffs
    return coeffs, forward(pad, k + blowup, evals_order)


def sparse_evaluate(indices, values, k, positions, evals_order=BITREV):
    """Exact outputs of forward() at the chosen positions for a coefficient vector with a few non-zeros."""
    pos = np.asarray(positions, dtype=np.uint64)
    idx = pos
    if evals_order == BITREV:
        idx = np.zeros_like(pos)
        for i in range(k):
            idx |= ((pos >> np.uint64(i)) & np.uint64(1)) << np.uint64(k - 1 - i)
    pts = domain_points(k, idx)
    chain = [pts[:, 1], pts[:, 0]]                  # y, x, pi(x), pi^2(x), ...
    for _ in range(2, k):
        t = chain[-1]
        chain.append((2 * (t * t % P) + P - 1) % P)
    out = np.zeros(len(pos), dtype=np.uint64)
    for j, v in zip(indices, values):
        term = np.full(len(pos), int(v) % P, dtype=np.uint64)
        for bit in range(k):
            if (int(j) >> bit) & 1:
                term = term * chain[bit] % P
        out = (out + term) % P
    return out.astype(np.uint32)
