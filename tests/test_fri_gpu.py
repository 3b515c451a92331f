"""GPU tests of the FRI calls (include/sppark_amd_fri.h) through sppark_amd.fri.  Field elements have one bit pattern, so
every comparison is exact.  Small cases are checked against the host model (tests/fri_model.py, whose domain is the oracle's
transform of X); the convention against the library's own transforms on the GPU (a fold of compute_ntt(c) is compute_ntt of the
folded coefficients); one large case per element size so that the grid is capped and a work-group takes several steps."""
import functools

import numpy as np
import pytest

import fri_model as FM

pytestmark = pytest.mark.gpu

EXPORTING = ["gl64", "bb31", "bb31x4", "bls12_381", "bn254", "bls12_377", "pallas", "vesta", "gl64_plonky2", "bb31_canonical"]
NTT_FIELDS = ["gl64", "bb31", "bls12_381", "bn254"]
LARGE = ["gl64", "bb31", "bb31x4", "bls12_381"]
CHUNK = 512                                                 # csrc/fri/fri_route.hpp FRI_RED_CHUNK


def _T(m):
    """csrc/fri/fri_route.hpp fri_tile_lg: log2 of the elements that 64 bytes per lane make"""
    return {4: 12, 8: 11, 16: 10, 32: 9}[m.f.w * np.dtype(m.f.dtype).itemsize]


@functools.lru_cache(maxsize=None)
def _model(field):
    return FM.FriModel(field)


def _dev(rows):
    import torch
    rows = np.array(rows)                                                # (a writable, contiguous copy)
    return torch.from_numpy(rows.view(np.int32 if rows.dtype == np.uint32 else np.int64)).cuda()


def _host(t, m):
    return t.cpu().numpy().view(m.f.dtype).reshape(-1, m.f.w)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(field, lg):
    """(wire rows with 0, 1 and p - 1 planted, their values, beta rows, a random shift row of the domain's field); never modified"""
    m = _model(field)
    n = 1 << lg
    x = m.random_rows(n, 9000 + lg)
    for j, edge in enumerate((0, m.f.one, m.f.pm1)):
        x[(3 * j + 1) % n] = edge
    x.setflags(write=False)
    return x, m.vals(x), m.random_rows(1, 41), m.base.random_rows(1, 43)


def _shift_arg(m, kind, shift_row):
    """(what fri takes, what the model takes)"""
    if kind == "none":
        return None, None
    if kind == "coset":
        return "coset", "coset"
    return m.base.f.shaped(shift_row.copy()), m.base.vals(shift_row)[0]


# ---- small cases against the model ----
@pytest.mark.parametrize("field", EXPORTING)
def test_fold_small(oracle, libs, field):
    from sppark_amd import fri
    m = _model(field)
    T = _T(m)
    k = 0
    for a in (1, 2, 3):
        for lg in sorted(set(range(a, 7)) | {T - 1, T, T + 1}):
            x, vals, beta, shift_row = _case(field, lg)
            for order in (fri.NATURAL, fri.BITREV):
                kind = ("none", "coset", "random")[k % 3]
                k += 1
                sh, sh_model = _shift_arg(m, kind, shift_row)
                want = m.rows(m.fold(vals, a, m.vals(beta)[0], sh_model, order))
                what = (field, a, lg, order, kind)
                d_in = _dev(x)
                d_out = _dev(np.full((1 << (lg - a), m.f.w), 5, dtype=m.f.dtype))
                b = _dev(beta) if k % 2 else m.f.shaped(beta.copy())                      # beta by device pointer / by value
                fri.fold(d_out, d_in, b, lg_arity=a, shift=sh, order=order, field=field, stream=_stream())
                assert (_host(d_out, m) == want).all(), what
                assert (_host(d_in, m) == x).all(), what
                out = np.full((1 << (lg - a), m.f.w), 5, dtype=m.f.dtype)                # host buffers
                fri.fold(m.f.shaped(out), m.f.shaped(x.copy()), m.f.shaped(beta.copy()), lg_arity=a, shift=sh, order=order, field=field)
                assert (out == want).all(), what
                if order == fri.NATURAL:                                                  # in place
                    fri.fold(d_in, d_in, b, lg_arity=a, shift=sh, order=order, field=field, stream=_stream())
                    got = _host(d_in, m)
                    h = 1 << (lg - a)
                    assert (got[:h] == want).all() and (got[h:] == x[h:]).all(), what


@pytest.mark.parametrize("field", EXPORTING)
def test_domain_small(oracle, libs, field):
    from sppark_amd import fri
    m = _model(field)
    T = _T(m)
    k = 0
    for lg in sorted(set(range(0, 7)) | {T - 1, T, T + 1}):
        _x, _vals, z_row, shift_row = _case(field, max(lg, 1))
        for order in (fri.NATURAL, fri.BITREV):
            kind = ("none", "coset", "random")[k % 3]
            k += 1
            sh, sh_model = _shift_arg(m, kind, shift_row)
            for z in (None, z_row):
                want = m.rows(m.domain_minus(lg, sh_model, order, None if z is None else m.vals(z)[0]))
                d_out = _dev(np.full((1 << lg, m.f.w), 5, dtype=m.f.dtype))
                zz = None if z is None else (_dev(z) if k % 2 else m.f.shaped(z.copy()))
                fri.domain(d_out, shift=sh, order=order, z=zz, field=field, stream=_stream())
                assert (_host(d_out, m) == want).all(), (field, lg, order, kind, z is None)


# ---- the convention: the library's own transforms as the yardstick ----
def _ntt(rows, order, field, m):
    """compute_ntt of the rows on the device (bb31x4: four component-wise bb31 transforms)"""
    import sppark_amd as S
    if not m.x4:
        d = _dev(rows)
        S.compute_ntt(0, d, order, S.NTTDirection.Forward, S.NTTType.Standard, field=field)
        return _host(d, m)
    out = np.empty_like(rows)
    for c in range(4):
        d = _dev(rows[:, c].copy())
        S.compute_ntt(0, d, order, S.NTTDirection.Forward, S.NTTType.Standard, field="bb31")
        out[:, c] = d.cpu().numpy().view(np.uint32)
    return out


@pytest.mark.parametrize("field", NTT_FIELDS + ["bb31x4"])
def test_fold_of_a_transform_is_the_transform_of_the_folded_coefficients(oracle, libs, field):
    import sppark_amd as S
    from sppark_amd import fri
    m = _model(field)
    lg = 12
    c = m.random_rows(1 << lg, 77)
    beta = m.random_rows(1, 78)
    cv, bv = m.vals(c), m.vals(beta)[0]
    for order, ntt_order in ((fri.NATURAL, S.NTTInputOutputOrder.NN), (fri.BITREV, S.NTTInputOutputOrder.NR)):
        ev = _dev(_ntt(c, ntt_order, field, m))
        for a in (1, 2, 3):
            out = _dev(np.zeros((1 << (lg - a), m.f.w), dtype=m.f.dtype))
            fri.fold(out, ev, _dev(beta), lg_arity=a, order=order, field=field, stream=_stream())
            want = _ntt(m.rows(m.fold_coeffs(cv, a, bv)), ntt_order, field, m)
            assert (_host(out, m) == want).all(), (field, order, a)


@pytest.mark.parametrize("field", NTT_FIELDS)
def test_fold_of_an_lde_and_the_domain_it_lies_on(oracle, libs, field):
    import sppark_amd as S
    from sppark_amd import fri
    m = _model(field)
    lg_dom, lg_blow = 6, 2
    lg = lg_dom + lg_blow
    x = m.random_rows(1 << lg_dom, 5)
    ext = np.zeros((1 << lg, m.f.w), dtype=m.f.dtype)
    ext[:1 << lg_dom] = x
    d_ext = _dev(ext)
    S.LDE(0, d_ext, lg_dom, lg_blow, field=field)
    beta = m.random_rows(1, 6)
    # the domain: the model's (the oracle's Coset transform of X), the library's, and the transform of X times the shift
    d_dom = _dev(np.zeros((1 << lg, m.f.w), dtype=m.f.dtype))
    fri.domain(d_dom, shift="coset", field=field, stream=_stream())
    assert (_host(d_dom, m) == m.rows(m.domain_minus(lg, "coset", FM.NATURAL))).all()
    for order, ntt_order in ((fri.NATURAL, S.NTTInputOutputOrder.NN), (fri.BITREV, S.NTTInputOutputOrder.NR)):
        xpoly = np.zeros((1 << lg, m.f.w), dtype=m.f.dtype)
        xpoly[1] = m.f.one
        pts = m.vals(_ntt(xpoly, ntt_order, field, m))
        g = m.base.vals(np.frombuffer(fri.coset_shift(field).tobytes(), dtype=m.f.dtype).reshape(1, -1))[0]
        assert g == m.coset_shift()
        fri.domain(d_dom, shift="coset", order=order, field=field, stream=_stream())
        assert (_host(d_dom, m) == m.rows([p * g % m.p for p in pts])).all(), (field, order)
    for a in (1, 2, 3):
        out = _dev(np.zeros((1 << (lg - a), m.f.w), dtype=m.f.dtype))
        fri.fold(out, d_ext, _dev(beta), lg_arity=a, shift="coset", order=fri.NATURAL, field=field, stream=_stream())
        want = m.rows(m.fold(m.vals(_host(d_ext, m)), a, m.vals(beta)[0], "coset", FM.NATURAL))
        assert (_host(out, m) == want).all(), (field, a)


# ---- one large case per element size ----
def _steps(m, lg, a, cus):
    """steps a work-group takes in an aligned fold, as csrc/fri/fri_route.hpp decides (tests/test_fri_route.py holds the route to
    these formulas): 2^(tile_bits - grid_lg)"""
    es = m.f.w * np.dtype(m.f.dtype).itemsize
    pack = max(16 // es, 1)
    acc = max((((1 << _T(m)) // 256) >> a) // pack, 1)
    out_lg = 8 + (acc * pack).bit_length() - 1
    tile_bits = max(lg - a - out_lg, 0)
    grid_lg = min(tile_bits, (cus * 8).bit_length() - 1, 12)
    return 1 << (tile_bits - grid_lg)


def _ntt_dev(d, order, field, m):
    """compute_ntt of a device tensor, out of place (bb31x4: four component-wise bb31 transforms)"""
    import torch
    import sppark_amd as S
    if not m.x4:
        d = d.clone()
        S.compute_ntt(0, d, order, S.NTTDirection.Forward, S.NTTType.Standard, field=field)
        return d
    cols = [d[:, c].contiguous() for c in range(4)]
    for col in cols:
        S.compute_ntt(0, col, order, S.NTTDirection.Forward, S.NTTType.Standard, field="bb31")
    return torch.stack(cols, dim=1)


@pytest.mark.parametrize("field", LARGE)
def test_fold_large(oracle, libs, field):
    """arity 3 at the smallest size at which the grid is capped and every work-group takes FOUR steps: the tile part of the
    twiddles advances three times and BITREV visits its tiles in an order that is not the natural one"""
    import torch
    import sppark_amd as S
    from sppark_amd import fri, poly
    m = _model(field)
    a = 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lg = next(k for k in range(a, 33) if _steps(m, k, a, cus) >= 4)
    assert _steps(m, lg, a, cus) == 4 and lg <= FM.TWO_ADICITY[field], (field, lg, cus)
    n = 1 << lg
    pool = _dev(m.random_rows(1 << 16, 123))
    g = torch.Generator(device="cuda"); g.manual_seed(2024)
    c = pool[torch.randint(0, 1 << 16, (n,), device="cuda", generator=g)]       # n canonical rows
    beta = m.random_rows(1, 124)
    b = m.vals(beta)[0]
    # the folded coefficients with the older vector calls: c[2k] + beta c[2k+1], three times with beta, beta^2, beta^4
    d = c
    for bl in (b, m.mul(b, b), m.mul(m.mul(b, b), m.mul(b, b))):
        pair = d.reshape(d.shape[0] // 2, 2, m.f.w)
        even, odd = pair[:, 0].contiguous(), pair[:, 1].contiguous()
        poly.vec_scale(odd, odd, m.f.shaped(m.rows([bl])), field=field)
        poly.vec_add(even, even, odd, field=field)
        d = even
    for order, ntt_order in ((fri.NATURAL, S.NTTInputOutputOrder.NN), (fri.BITREV, S.NTTInputOutputOrder.NR)):
        ev = _ntt_dev(c, ntt_order, field, m)
        out = torch.zeros((n >> a, m.f.w), dtype=c.dtype, device="cuda")
        fri.fold(out, ev, _dev(beta), lg_arity=a, order=order, field=field, stream=_stream())
        torch.cuda.synchronize()
        assert torch.equal(out, _ntt_dev(d, ntt_order, field, m)), (field, order, lg)
        del ev, out


def _offset_view(rows, pad):
    """the rows on the device, |pad| elements into a 16-byte aligned buffer"""
    import torch
    t = _dev(np.concatenate([np.zeros((pad, rows.shape[1]), dtype=rows.dtype), rows]))
    return t[pad:]


@pytest.mark.parametrize("field", ["gl64", "bb31"])
def test_fold_and_domain_on_pointers_that_miss_16_bytes(oracle, libs, field):
    """device tensors one element into an aligned buffer: the driver must take the element-wise instance"""
    from sppark_amd import fri
    m = _model(field)
    T = _T(m)
    for lg in (5, T + 2):
        x, vals, beta, shift_row = _case(field, lg)
        sh, sh_model = _shift_arg(m, "random", shift_row)
        for order in (fri.NATURAL, fri.BITREV):
            for a in (1, 3):
                want = m.rows(m.fold(vals, a, m.vals(beta)[0], sh_model, order))
                for pad_in, pad_out in ((1, 0), (0, 1), (1, 1)):
                    d_in = _offset_view(x, pad_in)
                    d_out = _offset_view(np.full((1 << (lg - a), m.f.w), 5, dtype=m.f.dtype), pad_out)
                    assert (d_in.data_ptr() % 16 != 0) == bool(pad_in) and (d_out.data_ptr() % 16 != 0) == bool(pad_out)
                    fri.fold(d_out, d_in, _dev(beta), lg_arity=a, shift=sh, order=order, field=field, stream=_stream())
                    assert (_host(d_out, m) == want).all(), (field, lg, order, a, pad_in, pad_out)
            want = m.rows(m.domain_minus(lg, sh_model, order, m.vals(beta)[0]))
            d_out = _offset_view(np.full((1 << lg, m.f.w), 5, dtype=m.f.dtype), 1)
            assert d_out.data_ptr() % 16 != 0
            fri.domain(d_out, shift=sh, order=order, z=_dev(beta), field=field, stream=_stream())
            assert (_host(d_out, m) == want).all(), (field, lg, order)


# ---- reduce ----
def _matrix(m, e, lg, width, layout, gap, seed):
    """(device buffer with non-canonical garbage in the gaps, the 2-D view fri takes, cols[j][i] as values)"""
    n = 1 << lg
    rows = e.random_rows(n * width, seed).reshape(width, n, e.f.w)
    rows[0, 0] = e.f.pm1
    garbage = np.iinfo(e.f.dtype).max
    lines, line = (width, n) if layout == "columns" else (n, width)
    buf = np.full((lines, line + gap, e.f.w), garbage, dtype=e.f.dtype)
    buf[:, :line] = rows if layout == "columns" else rows.transpose(1, 0, 2)
    d = _dev(buf.reshape(lines, -1))
    return d, d[:, :line * e.f.w], [e.vals(rows[j]) for j in range(width)]


@pytest.mark.parametrize("layout", ["columns", "rows"])
@pytest.mark.parametrize("field,base", [(f, False) for f in EXPORTING + ["m31"]] + [("bb31x4", True)])
def test_reduce(oracle, libs, field, base, layout):
    from sppark_amd import fri
    m = _model(field)
    e = m.base if base else m
    T = _T(e)
    shapes = [(w, 5) for w in (1, 2, 3, 5, 64, 257, CHUNK - 1, CHUNK, CHUNK + 1)] + [(3, 0), (3, 1), (5, T + 1), (64, T + 1)]
    if field not in ("gl64", "bb31", "bb31x4", "bls12_381", "m31"):
        shapes = [(3, 5), (CHUNK + 1, 1), (5, T + 1)]                   # the same code as a sibling library's: a sample
    for k, (width, lg) in enumerate(shapes):
        gap = (0, 4, 3)[k % 3]
        d_buf, view, cols = _matrix(m, e, lg, width, layout, gap, 100 + k)
        w = m.random_rows(width, 200 + k)
        sub, prev = m.random_rows(1, 300 + k), m.random_rows(1 << lg, 400 + k)
        for accumulate, sub_row in ((False, None), (True, sub)):
            want = m.rows(m.reduce(cols, m.vals(w), None if sub_row is None else m.vals(sub_row)[0],
                                   m.vals(prev) if accumulate else None, base=base))
            d_out = _dev(prev)
            fri.reduce(d_out, view, _dev(w), sub=None if sub_row is None else _dev(sub_row), accumulate=accumulate, layout=layout,
                       base=base, field=field, stream=_stream())
            assert (_host(d_out, m) == want).all(), (field, base, layout, width, lg, gap, accumulate)
            if k % 4 == 0:                                              # host buffers: staged, the gaps never copied
                out = prev.copy()
                hv = view.cpu().numpy()
                fri.reduce(m.f.shaped(out), hv, m.f.shaped(w.copy()), sub=None if sub_row is None else m.f.shaped(sub_row.copy()),
                           accumulate=accumulate, layout=layout, base=base, field=field)
                assert (out == want).all(), (field, base, layout, width, lg, gap, accumulate, "host")


@pytest.mark.parametrize("layout", ["columns", "rows"])
def test_reduce_lazy_sums_at_their_bound(oracle, libs, layout):
    """every matrix element and every weight component p - 1, 1025 columns: a 64-bit sum that is reduced too late wraps"""
    from sppark_amd import fri
    m = _model("bb31x4")
    width, lg, p = 1025, 5, m.p
    n = 1 << lg
    mat = _dev(np.full((width, n) if layout == "columns" else (n, width), p - 1, dtype=np.uint32))
    w = np.full((width, 4), p - 1, dtype=np.uint32)
    one_leaf = m.reduce([m.base.vals(np.full(1, p - 1, dtype=np.uint32))] * width, m.vals(w), base=True)
    d_out = _dev(np.zeros((n, 4), dtype=np.uint32))
    fri.reduce(d_out, mat, _dev(w), layout=layout, base=True, field="bb31x4", stream=_stream())
    assert (_host(d_out, m) == m.rows(one_leaf * n)).all()


@pytest.mark.parametrize("field,base", [("gl64", False), ("bb31", False), ("bls12_381", False), ("bb31x4", False), ("bb31x4", True)])
def test_deep_quotient(oracle, libs, field, base):
    from sppark_amd import fri
    m = _model(field)
    e = m.base if base else m
    lg, width = 10, 7
    d_buf, view, cols = _matrix(m, e, lg, width, "columns", 4, 55)
    w, value, z = m.random_rows(width, 56), m.random_rows(1, 57), m.random_rows(1, 58)
    zv = m.vals(z)[0]
    xs = m.domain(lg, "coset", FM.NATURAL)
    assert all(m.embed(x) != zv for x in xs)                             # z lies outside the domain
    num = m.reduce(cols, m.vals(w), m.vals(value)[0], base=base)
    for scratch in (None, _dev(np.zeros((1 << lg, m.f.w), dtype=m.f.dtype))):
        d_out = _dev(np.zeros((1 << lg, m.f.w), dtype=m.f.dtype))
        fri.deep_quotient(d_out, view, _dev(w), _dev(value), _dev(z), lg_n=lg, shift="coset", order=fri.NATURAL, layout="columns",
                          base=base, field=field, scratch=scratch, stream=_stream())
        got = m.vals(_host(d_out, m))
        # got = num / (x - z)  <=>  got * (x - z) = num: x - z is not zero and the field has no zero divisors
        assert [m.mul(q, m.sub(m.embed(x), zv)) for q, x in zip(got, xs)] == num, (field, base)


# ---- enqueue only: a fold and a reduce captured and replayed ----
@pytest.mark.parametrize("field", ["gl64", "bb31x4"])
def test_fold_and_reduce_are_captured(oracle, libs, field):
    import torch
    from sppark_amd import fri
    m = _model(field)
    base = field == "bb31x4"
    e = m.base if base else m
    lg, width = 12, 5
    x, _vals, beta, shift_row = _case(field, lg)
    d_in, d_beta = _dev(x), _dev(beta)
    shift = m.base.f.shaped(shift_row.copy())
    d_buf, view, _cols = _matrix(m, e, lg, width, "columns", 4, 66)
    d_w = _dev(m.random_rows(width, 67))
    direct_fold = _dev(np.zeros((1 << (lg - 2), m.f.w), dtype=m.f.dtype))
    direct_red = _dev(np.zeros((1 << lg, m.f.w), dtype=m.f.dtype))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                           # (also loads the kernels before the capture)
        fri.fold(direct_fold, d_in, d_beta, lg_arity=2, shift=shift, order=fri.BITREV, field=field, stream=s.cuda_stream)
        fri.reduce(direct_red, view, d_w, layout="columns", base=base, field=field, stream=s.cuda_stream)
    s.synchronize()
    out_fold, out_red = torch.zeros_like(direct_fold), torch.zeros_like(direct_red)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):                                  # a single stream, no parallel branches
        fri.fold(out_fold, d_in, d_beta, lg_arity=2, shift=shift, order=fri.BITREV, field=field, stream=s.cuda_stream)
        fri.reduce(out_red, view, d_w, layout="columns", base=base, field=field, stream=s.cuda_stream)
    assert not out_fold.any() and not out_red.any()                      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_fold, direct_fold) and torch.equal(out_red, direct_red)
