"""GPU tests of the field-vector arithmetic (sppark_field_add / sub / mul / scale / mul_sub), the polynomial product and the
vanishing quotient (include/sppark_amd_arith.h) through sppark_amd.poly.  Field elements have unique bit patterns, so every
comparison is exact.

Expected values of the pointwise operations are Python integers on the wire format (Montgomery words taken out of and put
back into Montgomery form as test_field_inverse_gpu.Info describes the formats); the product of the BabyBear quartic
extension, which this file does not re-derive, is the oracle's: prefix_op(MULTIPLY) on two-element arrays.  They are computed
once for a pool of a prime number of elements; an operand of any length is that pool repeated, and so is its expected
result -- the period shares no factor with a lane, access or tile size, so a misplaced element cannot go unnoticed."""
import functools

import numpy as np
import pytest

from test_field_inverse_gpu import FIELDS, WIDE, Info, _limbs

pytestmark = pytest.mark.gpu

# csrc/poly/vec_kernels.hpp vec_geom<F>::T: elements one work-group handles per iteration (256 lanes x U accesses x
# elements per 16-byte access), and VEC_WG_PER_CU, the grid's cap
VEC_T = {"gl64": 2048, "gl64_plonky2": 2048, "bb31": 4096, "bb31_canonical": 4096, "m31": 4096, "bb31x4": 1024}
VEC_WG_PER_CU = 8
OPS = ("add", "sub", "mul", "scale", "mul_sub", "mul_sub_k")
NTT_FIELDS = ("gl64", "bb31", "bls12_381", "bn254", "gl64_plonky2")


def _tile(field):
    return VEC_T.get(field, 512)


class Arith:
    """Python-integer arithmetic on rows of wire-format elements"""
    def __init__(self, field):
        import oracle as O
        self.O, self.f = O, Info(field)
        f = self.f
        self.x4 = f.w == 4 and not f.wide
        self.R = 1 if f.oname in ("gl64", "m31") else (1 << 256 if f.wide else 1 << 32)
        self.rinv = pow(self.R, -1, f.p)

    def ints(self, rows):
        if self.f.wide:
            return [sum(int(r[j]) << (64 * j) for j in range(4)) for r in rows]
        return [int(v) for v in rows.reshape(-1)]

    def rows(self, ints):
        f = self.f
        if f.wide:
            return np.array([_limbs(v) for v in ints], dtype=np.uint64).reshape(-1, 4)
        return np.array(ints, dtype=f.dtype).reshape(-1, f.w)

    def add(self, x, y):                                            # (componentwise for the extension)
        p = self.f.p
        return self.rows([(a + b) % p for a, b in zip(self.ints(x), self.ints(y))])

    def sub(self, x, y):
        p = self.f.p
        return self.rows([(a - b) % p for a, b in zip(self.ints(x), self.ints(y))])

    def mul(self, x, y):
        f = self.f
        if self.x4:
            out = np.empty_like(x)
            for i in range(len(x)):
                out[i] = self.O.prefix_op("bb31x4", np.stack([x[i], y[i]]), 1)[1]
            return out
        return self.rows([a * b * self.rinv % f.p for a, b in zip(self.ints(x), self.ints(y))])

    def value(self, row):                                           # the field element a wire row stands for (not the extension)
        return self.ints(row.reshape(1, -1))[0] * self.rinv % self.f.p

    def wire(self, v):
        return self.rows([v * self.R % self.f.p])[0]


class Data:
    """pools a, b, c of a prime number of canonical elements with the edge values planted, one k; never modified"""
    def __init__(self, field):
        self.field, self.ar = field, Arith(field)
        f = self.f = self.ar.f
        self.P = P = 307 if self.ar.x4 else 1009
        rng = np.random.default_rng(0x51 + len(field))
        pools = {}
        for name in "abck":
            if f.wide:
                x = rng.integers(0, 1 << 63, size=(P, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(P, 4), dtype=np.uint64)
                x[:, 3] &= np.uint64(0x0fffffffffffffff)                # < 2^252 < every modulus
            else:
                x = rng.integers(0, f.p, size=(P, f.w), dtype=np.uint64).astype(f.dtype)
            pools[name] = x
        zero = np.zeros(f.w, dtype=f.dtype)
        top = self.ar.rows([f.p - 1])[0] if not self.ar.x4 else np.full(4, f.p - 1, dtype=f.dtype)     # the largest canonical word(s)
        edge = [zero, f.one, f.pm1, top]
        if self.ar.x4:                                                  # a single non-zero component
            for j in range(4):
                e = zero.copy(); e[j] = f.dtype(f.p - 1 if j & 1 else 1 + j)
                edge.append(e)
        i = 0
        for x in edge:                                                  # every pair of edge values meets, with every edge value as c
            for y in edge:
                pools["a"][i], pools["b"][i], pools["c"][i] = x, y, edge[(i // 3) % len(edge)]
                i += 1
        assert i < P
        for x in pools.values():
            assert f.canonical(x).all()
            x.setflags(write=False)
        self.pools = pools
        self.k = pools["k"][:1]
        self._dev = {}

    @functools.lru_cache(maxsize=None)
    def small(self, name, shift=0):
        return np.roll(self.pools[name], -shift, axis=0)

    @functools.lru_cache(maxsize=None)
    def expected(self, op, a, b, c, shifts=(0, 0, 0)):
        """the pool-sized result of |op| on the pools named a, b, c (rolled by |shifts|)"""
        ar = self.ar
        x, y, z = self.small(a, shifts[0]), self.small(b, shifts[1]), self.small(c, shifts[2])
        K = np.repeat(self.k, self.P, axis=0)
        if op == "add": r = ar.add(x, y)
        elif op == "sub": r = ar.sub(x, y)
        elif op == "mul": r = ar.mul(x, y)
        elif op == "scale": r = ar.mul(x, K)
        else:
            r = ar.sub(ar.mul(x, y), z)
            if op == "mul_sub_k": r = ar.mul(r, K)
        r.setflags(write=False)
        return r

    def host(self, rows, n):
        return self.f.shaped(np.resize(rows, (n, self.f.w)))

    def dev(self, rows, n, key):
        """the pool repeated to n elements, built on the device"""
        import torch
        view = np.int32 if self.f.dtype == np.uint32 else np.int64
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(np.array(rows).view(view)).cuda()
        small = self._dev[key]
        idx = torch.arange(n, device="cuda") % self.P
        t = small[idx]
        return t.reshape(-1) if self.f.w == 1 else t


@functools.lru_cache(maxsize=None)
def _data(field):
    return Data(field)


def _call(op, out, a, b, c, k, field, stream=None):
    from sppark_amd import poly
    if op == "add": poly.vec_add(out, a, b, field=field, stream=stream)
    elif op == "sub": poly.vec_sub(out, a, b, field=field, stream=stream)
    elif op == "mul": poly.vec_mul(out, a, b, field=field, stream=stream)
    elif op == "scale": poly.vec_scale(out, a, k, field=field, stream=stream)
    elif op == "mul_sub": poly.vec_mul_sub(out, a, b, c, field=field, stream=stream)
    else: poly.vec_mul_sub(out, a, b, c, k=k, field=field, stream=stream)


def _operands(op):
    return 2 if op == "scale" else (4 if op.startswith("mul_sub") else 3)


def _lengths(T):
    return [1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5]


# (out, a, b, c): equal names are ONE buffer; "o": a buffer of its own
PLAIN = ("o", "a", "b", "c")
ALIAS = {2: [("a", "a", "b", "c")],
         3: [("a", "a", "b", "c"), ("b", "a", "b", "c"), ("o", "a", "a", "c"), ("a", "a", "a", "c")],
         4: [("a", "a", "b", "c"), ("b", "a", "b", "c"), ("c", "a", "b", "c"), ("o", "a", "a", "c"), ("a", "a", "a", "a")]}


def _run(D, op, pattern, n, on_device, k_on_device=False):
    """one call with the buffers of |pattern|; checks the result and that every buffer that is not out is unchanged"""
    import torch
    f = D.f
    names = pattern[:_operands(op)]
    names = names + tuple(names[1] for _ in range(4 - len(names)))         # (unused operands: any name)
    want = D.expected(op, names[1], names[2], names[3])
    bufs, orig = {}, {}
    for nm in set(pattern[:_operands(op)]):
        if on_device:
            bufs[nm] = torch.full_like(D.dev(D.small("a"), n, "a"), 5) if nm == "o" else D.dev(D.small(nm), n, nm).clone()
        else:
            bufs[nm] = np.full_like(D.host(D.small("a"), n), 5) if nm == "o" else D.host(D.small(nm), n).copy()
        if nm != "o":
            orig[nm] = bufs[nm].clone() if on_device else bufs[nm].copy()
    k = D.dev(D.k, 1, "k1") if k_on_device else f.shaped(D.k.copy())
    stream = torch.cuda.current_stream().cuda_stream if on_device else None
    _call(op, bufs[names[0]], bufs[names[1]], bufs[names[2]], bufs[names[3]], k, D.field, stream)
    what = (D.field, op, pattern, n, on_device, k_on_device)
    if on_device:
        torch.cuda.synchronize()
        assert torch.equal(bufs[names[0]], D.dev(want, n, (op,) + names[1:])), what
        for nm, o in orig.items():
            if nm != names[0]:
                assert torch.equal(bufs[nm], o), what
    else:
        assert (f.rows(bufs[names[0]]) == np.resize(want, (n, f.w))).all(), what
        for nm, o in orig.items():
            if nm != names[0]:
                assert (bufs[nm] == o).all(), what


@pytest.mark.parametrize("field", FIELDS)
def test_pointwise_host_arrays(oracle, libs, field):
    """every operation at every length around the access, lane and tile edges; every allowed aliasing"""
    D = _data(field)
    T = _tile(field)
    for n in _lengths(T):
        for op in OPS:
            _run(D, op, PLAIN, n, False)
    for n in (5, T + 1):
        for op in OPS:
            for pattern in ALIAS[_operands(op)]:
                _run(D, op, pattern, n, False)


@pytest.mark.parametrize("field", FIELDS)
def test_pointwise_device_tensors(oracle, libs, field):
    """the same on device tensors, k on the host and on the device, and one length above grid * T: the grid-stride
    loop wraps"""
    import torch
    D = _data(field)
    T = _tile(field)
    grid = torch.cuda.get_device_properties(0).multi_processor_count * VEC_WG_PER_CU
    for n in _lengths(T) + [grid * T + T + 3]:
        for op in OPS:
            _run(D, op, PLAIN, n, True)
    for n in (3, T + 1, 3 * T + 5):
        for op in ("scale", "mul_sub_k"):
            _run(D, op, PLAIN, n, True, k_on_device=True)
    for n in (5, T + 1):
        for op in OPS:
            for pattern in ALIAS[_operands(op)]:
                _run(D, op, pattern, n, True)


@pytest.mark.parametrize("field", ["gl64", "bb31", "m31"])
def test_pointwise_misaligned_views(oracle, libs, field):
    """a[1:], b[2:], out[3:] of 16-byte aligned allocations (c aligned): the element-wise instance; nothing outside the
    views changes"""
    import torch
    D = _data(field)
    f, T = D.f, _tile(field)
    stream = torch.cuda.current_stream().cuda_stream
    for n in (1, 2, 7, 257, T + 1, 3 * T + 5):
        A, B, C = (D.dev(D.small(nm), n + 8, nm).clone() for nm in "abc")
        assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0 and C.data_ptr() % 16 == 0
        keep = [A.clone(), B.clone(), C.clone()]
        for op in OPS:
            out = torch.full_like(A, 5)
            assert out.data_ptr() % 16 == 0
            _call(op, out[3:3 + n], A[1:1 + n], B[2:2 + n], C[:n], f.shaped(D.k.copy()), field, stream)
            torch.cuda.synchronize()
            want = D.dev(D.expected(op, "a", "b", "c", (1, 2, 0)), n, (op, "shifted"))
            assert torch.equal(out[3:3 + n], want), (field, op, n)
            assert (out[:3] == 5).all() and (out[3 + n:] == 5).all(), (field, op, n)
            assert torch.equal(A, keep[0]) and torch.equal(B, keep[1]) and torch.equal(C, keep[2]), (field, op, n)


def test_pointwise_in_stream_order(oracle, libs):
    """Goldilocks on a non-default stream: batched forward transform -> vec_mul -> inverse transform, all enqueued with
    device buffers, ONE synchronise at the end; against the oracle's transforms and Python integers"""
    import torch
    import sppark_amd
    from sppark_amd import poly
    O = oracle
    n, p = 1 << 10, O.GL64_P
    x = np.random.default_rng(77).integers(0, p, size=(2, n), dtype=np.uint64)
    d = torch.from_numpy(x.view(np.int64)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    sppark_amd.compute_ntt_batch(0, d, O.NR, O.FORWARD, O.STANDARD, "gl64", stream=s.cuda_stream)
    poly.vec_mul(d[0], d[0], d[1], field="gl64", stream=s.cuda_stream)
    sppark_amd.compute_ntt(0, d[0], O.RN, O.INVERSE, O.STANDARD, "gl64", stream=s.cuda_stream)
    s.synchronize()
    fa, fb = O.ntt_gl64(x[0], O.NR, O.FORWARD, O.STANDARD), O.ntt_gl64(x[1], O.NR, O.FORWARD, O.STANDARD)
    prod = np.array([int(u) * int(v) % p for u, v in zip(fa, fb)], dtype=np.uint64)
    want = O.ntt_gl64(prod, O.RN, O.INVERSE, O.STANDARD)
    got = d.cpu().numpy().view(np.uint64)
    assert (got[0] == want).all()
    assert (got[1] == fb).all()


# ---- polynomial product ----
def _random_rows(ar, n, seed):
    f = ar.f
    rng = np.random.default_rng(seed)
    if f.wide:
        x = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
        x[:, 3] &= np.uint64(0x0fffffffffffffff)
        return x
    return rng.integers(0, f.p, size=(n, f.w), dtype=np.uint64).astype(f.dtype)


def _evaluate(ar, coeffs, zs):
    return ar.f.rows(ar.O.poly_evaluate(ar.f.oname, ar.f.shaped(coeffs), ar.f.shaped(zs)))


PRODUCT_SHAPES = [(1, 1), (1, 5), (2, 1), (2, 2), (3, 2), (33, 32), (32, 33), (33, 33),       # 32 + 33 - 1 = 2^6, 33 + 33 - 1 = 2^6 + 1
                  (256, 257), (257, 257), (1024, 1025), (1025, 1025),                          # 2^9, 2^9 + 1, 2^11, 2^11 + 1
                  (5000, 3000)]


@pytest.mark.parametrize("field", NTT_FIELDS)
def test_product(oracle, libs, field):
    import torch
    from sppark_amd import poly
    ar = Arith(field)
    f = ar.f
    pool_a, pool_b = _random_rows(ar, 5000, 11), _random_rows(ar, 5000, 12)
    pool_a[0], pool_a[1], pool_b[0] = f.pm1, 0, f.one
    zs = _random_rows(ar, 8, 13)
    view = np.int32 if f.dtype == np.uint32 else np.int64
    cases = [(la, lb, False, False) for la, lb in PRODUCT_SHAPES] + [(33, 33, True, False), (700, 700, True, False),
                                                                     (5000, 3000, False, True), (257, 257, True, True)]
    for la, lb, square, on_device in cases:
        a, b = pool_a[:la].copy(), (pool_b[:lb].copy() if not square else None)
        lo = la + lb - 1
        out = np.full((lo + 16, f.w), 5, dtype=f.dtype)
        if on_device:
            da = torch.from_numpy(a.view(view)).cuda()
            db = da if square else torch.from_numpy(b.view(view)).cuda()
            do = torch.from_numpy(out.view(view)).cuda()
            poly.product(do, da, db, field=field, stream=torch.cuda.current_stream().cuda_stream)
            out = do.cpu().numpy().view(f.dtype).reshape(out.shape)
            assert (da.cpu().numpy().view(f.dtype).reshape(a.shape) == a).all()
        else:
            sa = f.shaped(a)
            sb = sa if square else f.shaped(b)
            so = f.shaped(out)
            poly.product(so, sa, sb, field=field)
            assert (f.rows(sa) == pool_a[:la]).all()
        if square:
            b = a
        what = (field, la, lb, square, on_device)
        assert (out[lo:] == 5).all(), what                              # the guard behind la + lb - 1
        got = out[:lo]
        assert f.canonical(got).all(), what
        if la <= 33 and lb <= 33:                                       # schoolbook in Python integers
            ia, ib, acc = ar.ints(a), ar.ints(b), [0] * lo
            for i, u in enumerate(ia):
                for j, v in enumerate(ib):
                    acc[i + j] += u * v
            assert (got == ar.rows([v * ar.rinv % f.p for v in acc])).all(), what
        assert (_evaluate(ar, got, zs) == ar.mul(_evaluate(ar, a, zs), _evaluate(ar, b, zs))).all(), what


# ---- vanishing quotient ----
def _oracle_ntt(O, field, x, order, direction, typ):
    if field.startswith("gl64"):
        return O.ntt_gl64(x.reshape(-1), order, direction, typ).reshape(-1, 1)
    if field.startswith("bb31"):
        return O.ntt_bb31(x.reshape(-1), order, direction, typ).reshape(-1, 1)
    return O.ntt_fr(O.CURVE_ID[field], x, order, direction, typ)


QUOTIENT_LGS = (0, 1, 2, 3, 6, 7, 9, 10, 11, 12, 13)


@pytest.mark.parametrize("field", NTT_FIELDS)
def test_vanishing_quotient_of_a_satisfied_system(oracle, libs, field):
    """c = a .* b: h is the exact quotient -- h[n-1] == 0 and A(z) B(z) - C(z) == h(z) (z^n - 1) at random z, with
    A, B, C from the oracle's inverse transform; in place and with the inputs left alone"""
    from sppark_amd import poly
    O = oracle
    ar = Arith(field)
    f = ar.f
    zs = _random_rows(ar, 8, 5)
    try:
        O.set_root_conventions(goldilocks_plonky2=field == "gl64_plonky2")
        for lg in QUOTIENT_LGS:
            n = 1 << lg
            a, b = _random_rows(ar, n, 100 + lg), _random_rows(ar, n, 200 + lg)
            c = ar.mul(a, b)
            sa, sb, sc = f.shaped(a.copy()), f.shaped(b.copy()), f.shaped(c.copy())
            h = np.full_like(sa, 5)
            poly.vanishing_quotient(h, sa, sb, sc, field=field)
            assert (f.rows(sa) == a).all() and (f.rows(sb) == b).all() and (f.rows(sc) == c).all(), (field, lg)
            hr = f.rows(h)
            assert f.canonical(hr).all() and not hr[n - 1].any(), (field, lg)
            A, B, C = (_oracle_ntt(O, field, v, O.NN, O.INVERSE, O.STANDARD) for v in (a, b, c))
            zn = zs
            for _ in range(lg):
                zn = ar.mul(zn, zn)
            zn1 = ar.sub(zn, np.repeat(f.one.reshape(1, -1), 8, axis=0))
            lhs = ar.sub(ar.mul(_evaluate(ar, A, zs), _evaluate(ar, B, zs)), _evaluate(ar, C, zs))
            assert (lhs == ar.mul(_evaluate(ar, hr, zs), zn1)).all(), (field, lg)
            if lg in (6, 12):                                           # h is a / h is b / h is c
                for which in range(3):
                    bufs = [f.shaped(a.copy()), f.shaped(b.copy()), f.shaped(c.copy())]
                    poly.vanishing_quotient(bufs[which], bufs[0], bufs[1], bufs[2], field=field)
                    assert (bufs[which] == h).all(), (field, lg, which)
                    for j, v in enumerate((a, b, c)):
                        assert j == which or (f.rows(bufs[j]) == v).all(), (field, lg, which, j)
    finally:
        O.set_root_conventions(False, False)


@pytest.mark.parametrize("field", ["gl64", "bls12_381"])
@pytest.mark.parametrize("lg", [3, 12])
def test_vanishing_quotient_is_the_composition_of_the_public_transforms(oracle, libs, field, lg):
    """random c: bit for bit what compute_ntt(NN, Inverse), compute_ntt(NN, Forward, Coset), (a .* b - c) / (g^n - 1) and
    compute_ntt(NN, Inverse, Coset) give, through the oracle's transforms and Python integers.  g^n: the oracle's forward
    coset transform of x^(n/2) has g^(n/2) as its element 0."""
    import torch
    from sppark_amd import poly
    O = oracle
    ar = Arith(field)
    f = ar.f
    n = 1 << lg
    a, b, c = (_random_rows(ar, n, 300 + lg + i) for i in range(3))
    mono = np.zeros((n, f.w), dtype=f.dtype)
    mono[n // 2] = f.one
    half = _oracle_ntt(O, field, mono, O.NN, O.FORWARD, O.COSET)[:1]
    gn = ar.value(ar.mul(half, half)[0])
    assert gn not in (0, 1)
    k = ar.wire(pow(gn - 1, -1, f.p)).reshape(1, -1)
    ev = [_oracle_ntt(O, field, _oracle_ntt(O, field, v, O.NN, O.INVERSE, O.STANDARD), O.NN, O.FORWARD, O.COSET) for v in (a, b, c)]
    t = ar.mul(ar.sub(ar.mul(ev[0], ev[1]), ev[2]), np.repeat(k, n, axis=0))
    want = _oracle_ntt(O, field, t, O.NN, O.INVERSE, O.COSET)
    h = np.full_like(f.shaped(a), 5)
    poly.vanishing_quotient(h, f.shaped(a), f.shaped(b), f.shaped(c), field=field)
    assert (f.rows(h) == want).all()
    view = np.int64
    da, db, dc = (torch.from_numpy(np.ascontiguousarray(v).view(view)).cuda() for v in (a, b, c))
    dh = torch.zeros_like(da)
    poly.vanishing_quotient(dh, da, db, dc, field=field, stream=torch.cuda.current_stream().cuda_stream)
    assert (dh.cpu().numpy().view(np.uint64).reshape(want.shape) == want).all()
    assert (da.cpu().numpy().view(np.uint64).reshape(a.shape) == a).all()
