"""GPU tests of the field-vector inverse and quotient (sppark_field_inverse / sppark_field_divide, the reference's
ff/batch_inversion.hpp) through sppark_amd.poly.  Field elements have unique bit patterns, so every comparison is exact.

The whole-array checks use nothing but the oracle's MULTIPLICATION: the inclusive product scan of the interleaved array
[x0, y0, x1, y1, ...] equals one at every odd index exactly when every x_i * y_i = 1 (induction over i), and that of
[q0, d0, 1/n0, q1, d1, 1/n1, ...] equals one at every third element exactly when every q_i * d_i = n_i.  Spot values come
from Python's pow(x, -1, p) and the oracle's own reciprocal."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WIDE = ("bls12_381", "bn254", "bls12_377", "pallas", "vesta")
FIELDS = ["gl64", "bb31"] + list(WIDE) + ["m31", "bb31x4", "gl64_plonky2", "bb31_canonical"]
ORACLE_NAME = {"gl64_plonky2": "gl64", "bb31_canonical": "bb31"}     # root-convention variants: the same field
GL64_P, BB31_P, M31_P = 0xffffffff00000001, 0x78000001, 0x7fffffff


def _limbs(v):
    return [(v >> (64 * j)) & 0xffffffffffffffff for j in range(4)]


class Info:
    """wire format of one field: elements as rows of |w| words of |dtype|"""
    def __init__(self, field):
        import oracle as O
        self.field, self.oname = field, ORACLE_NAME.get(field, field)
        base = self.oname
        self.tile = 1024 if (base in WIDE or base == "bb31x4") else 2048
        if base == "gl64":
            self.dtype, self.w, self.p, one, pm1 = np.uint64, 1, GL64_P, [1], [GL64_P - 1]
        elif base == "m31":
            self.dtype, self.w, self.p, one, pm1 = np.uint32, 1, M31_P, [1], [M31_P - 1]
        elif base == "bb31":                                            # Montgomery words, R = 2^32
            self.dtype, self.w, self.p, one, pm1 = np.uint32, 1, BB31_P, [(1 << 32) % BB31_P], [BB31_P - (1 << 32) % BB31_P]
        elif base == "bb31x4":
            self.dtype, self.w, self.p = np.uint32, 4, BB31_P
            one, pm1 = [(1 << 32) % BB31_P, 0, 0, 0], [BB31_P - (1 << 32) % BB31_P, 0, 0, 0]
        else:                                                           # Montgomery, R = 2^256, four 64-bit limbs
            self.dtype, self.w, self.p = np.uint64, 4, O.FR_MODULUS[O.CURVE_ID[base]]
            self.fid = O.FR_FIELD_ID[O.CURVE_ID[base]]
            one, pm1 = _limbs((1 << 256) % self.p), _limbs(self.p - (1 << 256) % self.p)
        self.one, self.pm1 = np.array(one, dtype=self.dtype), np.array(pm1, dtype=self.dtype)
        self.wide = base in WIDE

    def rows(self, a):
        return np.ascontiguousarray(a).reshape(-1, self.w)

    def is_zero(self, a):
        return (self.rows(a) == 0).all(axis=1)

    def canonical(self, a):
        r = self.rows(a)
        if not self.wide:
            return (r < self.dtype(self.p)).all(axis=1)                 # every component below p
        pl = _limbs(self.p)
        lt, eq = np.zeros(len(r), dtype=bool), np.ones(len(r), dtype=bool)
        for j in (3, 2, 1, 0):
            lt |= eq & (r[:, j] < np.uint64(pl[j]))
            eq &= r[:, j] == np.uint64(pl[j])
        return lt

    def shaped(self, rows):
        return rows.reshape(-1) if self.w == 1 else rows


@functools.lru_cache(maxsize=None)
def _pools(field):
    """(info, two pools of NON-ZERO canonical elements) of the largest length the tests use; never modified"""
    f = Info(field)
    n = 257 * f.tile + 77
    rng = np.random.default_rng(0x1f + len(field))
    pools = []
    for _ in range(2):
        if f.wide:                                                      # < 2^252 < every modulus, low bit set
            a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
            a[:, 3] &= np.uint64(0x0fffffffffffffff)
            a[:, 0] |= np.uint64(1)
        elif f.w == 4:
            a = rng.integers(0, f.p, size=(n, 4), dtype=np.uint64).astype(np.uint32)
            a[:, 0] = rng.integers(1, f.p, size=n, dtype=np.uint64).astype(np.uint32)
        else:
            a = rng.integers(1, f.p, size=n, dtype=np.uint64).astype(f.dtype)
        assert not f.is_zero(a).any() and f.canonical(a).all()          # the host-side premise of the skipped-pairs count
        a.setflags(write=False)
        pools.append(a)
    return f, pools[0], pools[1]


def _lengths(tile):
    return [1, 2, 3, 255, 256, 257, tile - 1, tile, tile + 1, 3 * tile + 5, 256 * tile, 256 * tile + 1, 257 * tile + 77]


def _zero_indices(n, tile):
    """index 0, the last, lane and tile boundaries, a whole lane, a whole tile, two adjacent ones -- where they exist"""
    e = tile // 256                                                     # elements per lane
    idx = {0, n - 1}
    if n > e: idx |= {e - 1, e}                                         # last of lane 0, first of lane 1
    if n > tile: idx |= {tile - 1, tile}                                # last of tile 0, first of tile 1
    if n > 12: idx |= {10, 11}                                          # two adjacent ones inside a lane
    if n >= 4 * e: idx |= set(range(3 * e, 4 * e))                      # lane 3 of tile 0
    if n >= 2 * tile: idx |= set(range(tile, 2 * tile))                 # tile 1
    if n >= 256 * tile: idx |= set(range(200 * tile + 7 * e, 200 * tile + 8 * e))      # a lane far into the spine
    return np.array(sorted(idx), dtype=np.int64)


def _check_inverse(O, f, x, y, planted):
    """y == 1/x element by element, 0 exactly at the |planted| zeros of x"""
    n = len(f.rows(x))
    zx = f.is_zero(x)
    assert int(zx.sum()) == planted
    assert (f.is_zero(y) == zx).all(), "zeros of the output are not exactly the zeros of the input"
    assert f.canonical(y).all(), "non-canonical output"
    keep = ~zx
    pairs = np.empty((2 * int(keep.sum()), f.w), dtype=f.dtype)
    pairs[0::2] = f.rows(x)[keep]
    pairs[1::2] = f.rows(y)[keep]
    assert n - len(pairs) // 2 == planted                               # nothing but the planted zeros left out
    if len(pairs):
        scan = f.rows(O.prefix_op(f.oname, f.shaped(pairs), 1))
        assert (scan[1::2] == f.one).all(), "x * y != 1 somewhere"


def _expected_inverse(O, f, xi):
    """independent value of 1/xi for one element (None: no independent source for this field)"""
    if not xi.any():
        return np.zeros(f.w, dtype=f.dtype)
    if f.oname in ("gl64", "m31"):
        return np.array([pow(int(xi[0]), -1, f.p)], dtype=f.dtype)
    if f.oname == "bb31":
        return np.array([pow(int(xi[0]), -1, f.p) * (1 << 64) % f.p], dtype=f.dtype)       # 1/a * R^2 on the Montgomery word
    if f.wide:
        return O.field_op(f.fid, 3, xi)
    return None


def _spot_check(O, f, x, y, seed):
    n = len(f.rows(x))
    idx = list(range(n)) if n <= 16 else [0, n - 1] + list(np.random.default_rng(seed).choice(np.arange(1, n - 1), 14, replace=False))
    for i in idx:
        want = _expected_inverse(O, f, f.rows(x)[i])
        if want is not None:
            assert (f.rows(y)[i] == want).all(), (f.field, n, int(i))


@pytest.mark.parametrize("field", FIELDS)
def test_field_inverse_vs_oracle(oracle, libs, field):
    """lengths around the lane / tile / spine edges; zero-free, zeros at every edge, all zero; in place"""
    from sppark_amd import poly
    O = oracle
    f, pool, _ = _pools(field)
    for n in _lengths(f.tile):
        # zero-free, with one and p-1 (its own inverse) planted
        x = pool[:n].copy()
        if n >= 3:
            f.rows(x)[n // 3] = f.one
            f.rows(x)[2 * n // 3] = f.pm1
        x0 = x.copy()
        y = np.zeros_like(x)
        poly.inverse(y, x, field=field)
        assert (x == x0).all()                                          # the input is left alone
        _check_inverse(O, f, x, y, 0)
        _spot_check(O, f, x, y, n)
        if n >= 3:
            assert (f.rows(y)[n // 3] == f.one).all() and (f.rows(y)[2 * n // 3] == f.pm1).all()
        # zeros at every edge
        zi = _zero_indices(n, f.tile)
        xz = x.copy()
        f.rows(xz)[zi] = 0
        yz = np.zeros_like(xz)
        poly.inverse(yz, xz, field=field)
        _check_inverse(O, f, xz, yz, len(zi))
        _spot_check(O, f, xz, yz, n + 1)
        keep = ~f.is_zero(xz)
        assert (f.rows(yz)[keep] == f.rows(y)[keep]).all()              # the zeros change nothing around them
        # in place
        w = xz.copy()
        poly.inverse(w, w, field=field)
        assert (w == yz).all(), (field, n, "in place")
        if n in (3, f.tile + 1):                                        # the whole array zero
            z = np.zeros_like(x)
            out = np.full_like(x, 5)
            poly.inverse(out, z, field=field)
            assert not out.any(), (field, n, "all zero")


@pytest.mark.parametrize("field", FIELDS)
def test_field_divide_vs_oracle(oracle, libs, field):
    """out * den == num through the oracle's multiplication; zero denominators; out aliasing num, den, both"""
    from sppark_amd import poly
    O = oracle
    f, pool, pool2 = _pools(field)
    for n in _lengths(f.tile):
        num = pool2[:n].copy()
        den = pool[:n].copy()
        zi = _zero_indices(n, f.tile) if n > 2 else np.array([], dtype=np.int64)
        f.rows(den)[zi] = 0
        ninv = np.zeros_like(num)
        poly.inverse(ninv, num, field=field)
        _check_inverse(O, f, num, ninv, 0)                              # 1/num, verified before it is used below
        q = np.zeros_like(num)
        poly.divide(q, num, den, field=field)
        zd = f.is_zero(den)
        assert int(zd.sum()) == len(zi)
        assert (f.is_zero(q) == zd).all() and f.canonical(q).all()
        keep = ~zd
        tri = np.empty((3 * int(keep.sum()), f.w), dtype=f.dtype)
        tri[0::3] = f.rows(q)[keep]
        tri[1::3] = f.rows(den)[keep]
        tri[2::3] = f.rows(ninv)[keep]
        assert n - len(tri) // 3 == len(zi)
        if len(tri):
            scan = f.rows(O.prefix_op(f.oname, f.shaped(tri), 1))
            assert (scan[2::3] == f.one).all(), "out * den != num somewhere"
        # out is num / out is den
        a = num.copy()
        poly.divide(a, a, den, field=field)
        assert (a == q).all(), (field, n, "out is num")
        b = den.copy()
        poly.divide(b, num, b, field=field)
        assert (b == q).all(), (field, n, "out is den")
        # x / x: one wherever x != 0, zero elsewhere
        c = den.copy()
        poly.divide(c, c, c, field=field)
        assert (f.rows(c)[keep] == f.one).all() and not f.rows(c)[zd].any(), (field, n, "x / x")


@pytest.mark.parametrize("field", FIELDS)
def test_field_inverse_device_buffers(libs, field):
    """torch device tensors on torch's current stream, at the largest length: the bytes of the host run"""
    import torch
    from sppark_amd import poly
    f, pool, pool2 = _pools(field)
    n = _lengths(f.tile)[-1]
    den = pool[:n].copy()
    f.rows(den)[_zero_indices(n, f.tile)] = 0
    num = pool2[:n].copy()
    want_inv, want_div = np.zeros_like(den), np.zeros_like(den)
    poly.inverse(want_inv, den, field=field)
    poly.divide(want_div, num, den, field=field)
    assert f.is_zero(want_inv).sum() == f.is_zero(den).sum() and want_inv.any() and want_div.any()
    view = np.int32 if f.dtype == np.uint32 else np.int64
    s = torch.cuda.current_stream().cuda_stream

    def back(t):
        return t.cpu().numpy().view(f.dtype).reshape(den.shape)

    d_den, d_num = torch.from_numpy(den.view(view)).cuda(), torch.from_numpy(num.view(view)).cuda()
    d_out = torch.zeros_like(d_den)
    poly.inverse(d_out, d_den, field=field, stream=s)
    torch.cuda.synchronize()
    assert (back(d_out) == want_inv).all() and (back(d_den) == den).all()
    d_out = torch.zeros_like(d_den)
    poly.divide(d_out, d_num, d_den, field=field, stream=s)
    torch.cuda.synchronize()
    assert (back(d_out) == want_div).all() and (back(d_den) == den).all() and (back(d_num) == num).all()
    poly.divide(d_num, d_num, d_den, field=field, stream=s)            # out is num
    torch.cuda.synchronize()
    assert (back(d_num) == want_div).all()
    poly.inverse(d_den, d_den, field=field, stream=s)                  # in place
    torch.cuda.synchronize()
    assert (back(d_den) == want_inv).all()


def test_field_inverse_round_trip_full_size(libs):
    """Goldilocks, 2^24 elements (the NTT's BASELINE size): 1/(1/x) == x, and the quotients of consecutive
    prefix products give the input back.  Exact, no oracle."""
    from sppark_amd import poly
    n = 1 << 24
    x = np.random.default_rng(24).integers(1, GL64_P, size=n, dtype=np.uint64)
    y = np.zeros_like(x)
    poly.inverse(y, x, field="gl64")
    assert (y != 0).all() and (y < np.uint64(GL64_P)).all()
    for i in (0, 1, n // 2, n - 1):
        assert int(y[i]) == pow(int(x[i]), -1, GL64_P)
    back = np.zeros_like(x)
    poly.inverse(back, y, field="gl64")
    assert (back == x).all()
    p = np.zeros_like(x)
    poly.prefix_op(p, x, poly.MULTIPLY, field="gl64")
    q = np.zeros(n - 1, dtype=np.uint64)
    poly.divide(q, p[1:].copy(), p[:-1].copy(), field="gl64")           # (copies: views of one array overlap partially -- rejected)
    with pytest.raises(Exception, match="overlap"):
        poly.divide(q, p[1:], p[:-1], field="gl64")
    assert p[0] == x[0] and (q == x[1:]).all()
