"""GPU tests of the multilinear tables and sumcheck rounds (include/sppark_amd_mle.h) through sppark_amd.mle.  Field elements
have unique bit patterns, so every comparison is exact.

Expected values are Python integers on the wire format (tests/mle_model.py).  Small tables go through the whole model.  Large
ones need no big model: a fold or a round of a table that repeats a pool of an odd prime number of elements is periodic in
the pool (the sums are counts per residue class times the class's term), and evaluate is checked on three tables -- a
repeated pool of 2^m elements (blind to the high index bits), a table constant on blocks (blind to the low ones) and zeros
with planted elements around every lane, wave, tile and grid-stride boundary (sees a misplaced element)."""
import functools
import threading

import numpy as np
import pytest

import mle_model as M
from test_field_inverse_gpu import FIELDS

pytestmark = pytest.mark.gpu

# csrc/mle/mle_route.hpp mle_tile_lg: log2 elements of a tile, by element size (4 / 8 / 16 / 32 bytes), and MLE_WG_PER_CU
MLE_T = {"gl64": 11, "gl64_plonky2": 11, "bb31": 12, "bb31_canonical": 12, "m31": 12, "bb31x4": 10}
MLE_WG_PER_CU = 8
LARGE_FIELDS = ["gl64", "bb31", "bb31x4", "bls12_381"]
FORMS = [(M.PRODUCT, 1), (M.PRODUCT, 2), (M.PRODUCT, 3), (M.PRODUCT, 4), (M.EQ_MUL_SUB, 4)]
MAX_LARGE_LG = 24


def _T(field):
    return MLE_T.get(field, 9)


@functools.lru_cache(maxsize=None)
def _model(field):
    return M.Model(field)


def _dev(m, rows):
    import torch
    f = m.f
    t = torch.from_numpy(np.array(rows).view(np.int32 if f.dtype == np.uint32 else np.int64)).cuda()      # (a writable copy)
    return t.reshape(-1) if f.w == 1 else t.reshape(-1, f.w)


def _back(m, t):
    return t.cpu().numpy().view(m.f.dtype).reshape(-1, m.f.w)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(field, lg):
    """four tables as wire rows with the edge values planted, their values, a point -- never modified"""
    m = _model(field)
    n = 1 << lg
    rows = [m.random_rows(n, 2000 * lg + k) for k in range(4)]
    for k, x in enumerate(rows):
        for j, edge in enumerate((0, m.f.one, m.f.pm1)):
            x[(j + k) % n] = edge
        assert m.f.canonical(x).all()
        x.setflags(write=False)
    point = m.random_rows(max(lg, 1), 99 + lg)
    point.setflags(write=False)
    return rows, [m.vals(x) for x in rows], point


@functools.lru_cache(maxsize=None)
def _want_fold(field, lg, order):
    m = _model(field)
    rows, vals, point = _case(field, lg)
    return m.rows(m.fold(vals[0], m.vals(point[:1])[0], order))


@functools.lru_cache(maxsize=None)
def _want_point(field, lg):
    m = _model(field)
    rows, vals, point = _case(field, lg)
    pv = m.vals(point)[:lg]
    return m.rows(m.eq(pv)), m.row(m.evaluate(vals[0], pv))


@functools.lru_cache(maxsize=None)
def _want_round(field, lg, form, nt, order):
    m = _model(field)
    rows, vals, point = _case(field, lg)
    return m.rows(m.round(vals[:nt], form, order))


def _odd_view(m, rows):
    """a device view that starts one element into a 16-byte aligned allocation (single-word fields: the element-wise instance)"""
    import torch
    t = _dev(m, rows)
    big = torch.zeros((t.shape[0] + 8,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[1:1 + t.shape[0]] = t
    return big[1:1 + t.shape[0]], big


# ---- dense random tables, whole model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", FIELDS)
def test_dense_fold_evaluate_eq(oracle, libs, field):
    """every lg_n up to T + 2: host and device buffers, r and point on the host and on the device, a device view at an odd
    element offset; inputs are left alone"""
    import torch
    from sppark_amd import mle
    m = _model(field)
    f = m.f
    for lg in range(0, _T(field) + 3):
        rows, vals, point = _case(field, lg)
        n = 1 << lg
        tab, pt = f.shaped(rows[0].copy()), f.shaped(point[:max(lg, 1)].copy())
        d_tab, d_pt = _dev(m, rows[0]), _dev(m, point)
        odd, whole = _odd_view(m, rows[0])
        want_eq, want_ev = _want_point(field, lg)
        # evaluate: host / device table, host / device point, odd view
        for table, p in ((tab, pt[:lg] if f.w == 1 else pt[:lg]), (d_tab, pt[:lg]), (d_tab, d_pt[:lg]), (odd, d_pt[:lg]), (tab, d_pt[:lg])):
            got = mle.evaluate(table, p if lg else p[:0], field=field, stream=_stream())
            assert (got == want_ev).all(), (field, lg, "evaluate")
        assert (f.rows(tab) == rows[0]).all() and (_back(m, d_tab) == rows[0]).all() and (_back(m, odd) == rows[0]).all()
        # eq: host / device out, host / device point, odd view with guards around it
        out = np.full_like(tab, 5)
        mle.eq(out, pt[:lg], field=field)
        assert (f.rows(out) == want_eq).all(), (field, lg, "eq host")
        d_out = torch.full_like(d_tab, 5)
        mle.eq(d_out, d_pt[:lg], field=field, stream=_stream())
        assert (_back(m, d_out) == want_eq).all(), (field, lg, "eq device")
        whole.fill_(5)
        mle.eq(odd, pt[:lg], field=field, stream=_stream())
        assert (_back(m, odd) == want_eq).all() and (whole[:1] == 5).all() and (whole[1 + n:] == 5).all(), (field, lg, "eq odd view")
        if lg == 0:
            continue
        # fold
        r, d_r = f.shaped(point[:1].copy()), d_pt[:1]
        for order in (M.LOW, M.HIGH):
            want = _want_fold(field, lg, order)
            out = np.full((n // 2, f.w), 5, dtype=f.dtype)
            mle.fold(f.shaped(out), tab, r, order=order, field=field)
            assert (out == want).all(), (field, lg, order, "fold host")
            odd, whole = _odd_view(m, rows[0])
            for table, rr in ((d_tab, r), (d_tab, d_r), (odd, d_r)):
                d_out = torch.full_like(d_tab[:n // 2], 5)
                mle.fold(d_out, table, rr, order=order, field=field, stream=_stream())
                torch.cuda.synchronize()
                assert (_back(m, d_out) == want).all(), (field, lg, order, "fold device")
            d_guard = torch.full_like(whole, 5)                 # out at an odd offset too
            mle.fold(d_guard[3:3 + n // 2], odd, r, order=order, field=field, stream=_stream())
            torch.cuda.synchronize()
            assert (_back(m, d_guard[3:3 + n // 2]) == want).all() and (d_guard[:3] == 5).all() and (d_guard[3 + n // 2:] == 5).all()
        assert (f.rows(tab) == rows[0]).all() and (_back(m, d_tab) == rows[0]).all() and (_back(m, odd) == rows[0]).all()


def _round_shapes(field, lg):
    return FORMS if lg <= 5 or lg == _T(field) + 1 else [(M.PRODUCT, 2), (M.EQ_MUL_SUB, 4)]


@pytest.mark.parametrize("field", FIELDS)
def test_dense_round(oracle, libs, field):
    """every lg_n up to T + 2, both orders; every table count and both forms at the small sizes and one above a tile; host
    tables, device tables, a mix, and device views at an odd element offset"""
    from sppark_amd import mle
    m = _model(field)
    f = m.f
    for lg in range(1, _T(field) + 3):
        rows, vals, point = _case(field, lg)
        host = [f.shaped(x.copy()) for x in rows]
        dev = [_dev(m, x) for x in rows]
        odd = [_odd_view(m, x)[0] for x in rows]
        for form, nt in _round_shapes(field, lg):
            for order in (M.LOW, M.HIGH):
                want = _want_round(field, lg, form, nt, order)
                mixed = [dev[k] if k & 1 else host[k] for k in range(nt)]
                for tables in (host[:nt], dev[:nt], mixed, odd[:nt]):
                    got = mle.round(tables, form=form, order=order, field=field, stream=_stream())
                    assert got.shape == want.shape and (got == want).all(), (field, lg, form, nt, order)
        for k in range(4):
            assert (f.rows(host[k]) == rows[k]).all() and (_back(m, dev[k]) == rows[k]).all()


# ---- large sizes -----------------------------------------------------------------------------------------------------------
def _large_lgs(field):
    """every lg_n at which the route's launch count changes, and the least at which a work-group loops over tiles"""
    import torch
    T = _T(field)
    cap = torch.cuda.get_device_properties(0).multi_processor_count * MLE_WG_PER_CU
    loops = T + cap.bit_length()                                # least lg with 2^lg > cap * 2^T
    lgs = {T + 1, 2 * T + 1, loops}
    assert loops <= MAX_LARGE_LG, "a device this large needs a larger table for the grid-stride case"
    return sorted(lg for lg in lgs if lg <= MAX_LARGE_LG)


@functools.lru_cache(maxsize=None)
def _pool(field):
    """a pool of an odd prime number of canonical elements with the edge values planted, as rows, values and on the device"""
    m = _model(field)
    P = 307 if m.x4 else 1009
    rows = m.random_rows(P, 0x77 + len(field))
    rows[0], rows[1], rows[2] = 0, m.f.one, m.f.pm1
    rows.setflags(write=False)
    return P, rows, m.vals(rows), _dev(m, rows)


def _repeat(small, n, shift=0):
    """table[i] = small[(i + shift) mod len(small)], built on the device"""
    import torch
    idx = (torch.arange(n, device="cuda") + shift) % small.shape[0]
    return small[idx]


@pytest.mark.parametrize("field", LARGE_FIELDS)
def test_large_fold_and_round(oracle, libs, field):
    import torch
    from sppark_amd import mle
    m = _model(field)
    P, rows, vals, small = _pool(field)
    r_rows = m.random_rows(1, 5)
    r = m.vals(r_rows)[0]
    shifts = (0, 37, 101, 500 % P)
    for lg in _large_lgs(field):
        n, h = 1 << lg, 1 << (lg - 1)
        tables = [_repeat(small, n, s) for s in shifts]
        for order in (M.LOW, M.HIGH):
            # pair i of the table shifted by s: a function of i mod P
            def pair(c, s):
                return (vals[(2 * c + s) % P], vals[(2 * c + 1 + s) % P]) if order == M.LOW else (vals[(c + s) % P], vals[(c + h + s) % P])
            want = _dev(m, m.rows([m.line(*pair(c, 0), r) for c in range(P)]))
            out = torch.zeros_like(tables[0][:h])
            mle.fold(out, tables[0], m.f.shaped(r_rows.copy()), order=order, field=field, stream=_stream())
            torch.cuda.synchronize()
            assert torch.equal(out, _repeat(want, h)), (field, lg, order, "fold")
            del out
            for form, nt in ((M.PRODUCT, 2), (M.EQ_MUL_SUB, 4), (M.PRODUCT, 3)):
                d = m.degree(form, nt)
                s_want = [m.zero] * (d + 1)
                for c in range(P):
                    count = h // P + (1 if c < h % P else 0)
                    ps = [pair(c, s) for s in shifts[:nt]]
                    terms = m.pair_terms(form, [p[0] for p in ps], [p[1] for p in ps])
                    s_want = [m.add(x, m.smul(count, y)) for x, y in zip(s_want, terms)]
                got = mle.round(tables[:nt], form=form, order=order, field=field, stream=_stream())
                assert (got == m.rows(s_want)).all(), (field, lg, order, form, nt)
        del tables


def _planted_indices(field, lg, rng):
    import torch
    T = _T(field)
    n = 1 << lg
    es = _model(field).f.w * np.dtype(_model(field).f.dtype).itemsize
    N = max(16 // es, 1)
    cap = torch.cuda.get_device_properties(0).multi_processor_count * MLE_WG_PER_CU
    idx = {0, n - 1}
    for edge in (N, 64 * N, 256 * N, 1 << T, 2 << T, cap << T, n // 2, n - (1 << T)):      # access, wave, lane block, tile, grid stride
        for i in (edge - 1, edge):
            if 0 <= i < n:
                idx.add(i)
    idx |= {int(i) for i in rng.integers(0, n, size=64)}
    return sorted(idx)


@pytest.mark.parametrize("field", LARGE_FIELDS)
def test_large_evaluate_and_eq(oracle, libs, field):
    import torch
    from sppark_amd import mle, poly
    m = _model(field)
    f = m.f
    mm = 10
    pool_rows = m.random_rows(1 << mm, 0x99)
    pool_vals, d_pool = m.vals(pool_rows), _dev(m, pool_rows)
    for lg in _large_lgs(field):
        n = 1 << lg
        rng = np.random.default_rng(lg)
        point = m.random_rows(lg, 0x55 + lg)
        pv, d_point = m.vals(point), _dev(m, point)
        # (a) the pool repeated: only the low mm variables matter
        t = _repeat(d_pool, n)
        assert (mle.evaluate(t, d_point, field=field, stream=_stream()) == m.row(m.evaluate(pool_vals, pv[:mm]))).all(), (field, lg, "a")
        # (b) constant on blocks of 2^(lg - mm): only the high mm variables matter
        t = d_pool[torch.arange(n, device="cuda") >> (lg - mm)]
        keep = t.clone()
        assert (mle.evaluate(t, f.shaped(point.copy()), field=field, stream=_stream()) == m.row(m.evaluate(pool_vals, pv[lg - mm:]))).all(), (field, lg, "b")
        assert torch.equal(t, keep)
        del keep
        # (c) zeros with planted elements
        idx = _planted_indices(field, lg, rng)
        planted = m.random_rows(len(idx), 0x33 + lg)
        planted[~planted.any(axis=1)] = f.one                   # non-zero
        assert f.canonical(planted).all()
        t.zero_()
        t[torch.tensor(idx, device="cuda")] = _dev(m, planted)
        eq_at = [m.eq_at(pv, i) for i in idx]
        want = m.total(m.mul(v, e) for v, e in zip(m.vals(planted), eq_at))
        assert (mle.evaluate(t, d_point, field=field, stream=_stream()) == m.row(want)).all(), (field, lg, "c")
        # eq: the whole table against doubling with vec_scale from the model's 2^mm table, and the planted indices
        mle.eq(t, d_point, field=field, stream=_stream())
        cur, hi, lo = _dev(m, m.rows(m.eq(pv[:mm]))), None, None
        for j in range(mm, lg):
            hi = torch.empty_like(cur)
            poly.vec_scale(hi, cur, f.shaped(point[j:j + 1].copy()), field=field, stream=_stream())
            lo = torch.empty_like(cur)
            poly.vec_scale(lo, cur, f.shaped(m.rows([m.sub(m.one, pv[j])])), field=field, stream=_stream())
            cur = torch.cat([lo, hi])
        torch.cuda.synchronize()
        assert torch.equal(t, cur), (field, lg, "eq")
        got = _back(m, t[torch.tensor(idx, device="cuda")])
        assert (got == m.rows(eq_at)).all(), (field, lg, "eq planted")
        del t, cur, hi, lo


# ---- aliasing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["gl64", "bb31", "bb31x4", "bls12_381", "m31"])
def test_aliasing(oracle, libs, field):
    import torch
    from sppark_amd import mle
    m = _model(field)
    f = m.f
    for lg in (1, 4, _T(field) + 1):
        rows, vals, point = _case(field, lg)
        h = 1 << (lg - 1)
        want = _want_fold(field, lg, M.HIGH)
        r = f.shaped(point[:1].copy())
        tab = f.shaped(rows[0].copy())                          # HIGH in place: the first half is overwritten, the second kept
        mle.fold(tab, tab, r, order=M.HIGH, field=field)
        assert (f.rows(tab)[:h] == want).all() and (f.rows(tab)[h:] == rows[0][h:]).all(), (field, lg)
        d_tab = _dev(m, rows[0])
        mle.fold(d_tab, d_tab, r, order=M.HIGH, field=field, stream=_stream())
        torch.cuda.synchronize()
        assert (_back(m, d_tab)[:h] == want).all() and (_back(m, d_tab)[h:] == rows[0][h:]).all(), (field, lg)
        # a round whose tables are all one buffer: the sum of squares of the pair lines
        d_tab = _dev(m, rows[0])
        for order in (M.LOW, M.HIGH):
            want_sq = m.rows(m.round([vals[0], vals[0]], M.PRODUCT, order))
            assert (mle.round([d_tab, d_tab], order=order, field=field, stream=_stream()) == want_sq).all(), (field, lg, order)
            host = f.shaped(rows[0].copy())
            assert (mle.round([host, host], order=order, field=field) == want_sq).all(), (field, lg, order)
        # evaluate leaves its input alone
        before = d_tab.clone()
        mle.evaluate(d_tab, f.shaped(point[:lg].copy()), field=field, stream=_stream())
        assert torch.equal(d_tab, before)


# ---- streams and threads -------------------------------------------------------------------------------------------------------
def test_folds_in_stream_order(oracle, libs):
    """two folds enqueued on a non-default stream with device buffers (r on the device too), ONE synchronise at the end"""
    import torch
    from sppark_amd import mle
    field = "gl64"
    m = _model(field)
    lg = _T(field) + 2
    rows, vals, point = _case(field, lg)
    rv = m.vals(point[:2])
    want = m.rows(m.fold(m.fold(vals[0], rv[0], M.LOW), rv[1], M.HIGH))
    d_tab, d_pt = _dev(m, rows[0]), _dev(m, point)
    mid = torch.zeros_like(d_tab[:1 << (lg - 1)])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    mle.fold(mid, d_tab, d_pt[0:1], order=M.LOW, field=field, stream=s.cuda_stream)
    mle.fold(mid, mid, d_pt[1:2], order=M.HIGH, field=field, stream=s.cuda_stream)
    s.synchronize()
    assert (_back(m, mid)[:1 << (lg - 2)] == want).all()
    assert (_back(m, d_tab) == rows[0]).all()


def test_rounds_from_two_threads(oracle, libs):
    from sppark_amd import mle
    field = "gl64"
    m = _model(field)
    lgs = (_T(field) + 2, _T(field) + 1)
    dev = [[_dev(m, x) for x in _case(field, lg)[0][:2]] for lg in lgs]
    want = [_want_round(field, lg, M.PRODUCT, 2, M.LOW) for lg in lgs]
    got, errors = [None, None], []

    def work(k):
        try:
            for _ in range(8):
                got[k] = mle.round(dev[k], field=field)
                assert (got[k] == want[k]).all()
        except Exception as e:                                  # noqa: BLE001 (reported below, in the main thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


# ---- the protocol, end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [M.LOW, M.HIGH])
@pytest.mark.parametrize("form", [M.PRODUCT, M.EQ_MUL_SUB])
@pytest.mark.parametrize("field", ["gl64", "bb31x4", "bls12_381"])
def test_sumcheck_protocol(oracle, libs, field, form, order):
    """A whole sumcheck at lg_n = T + 3 on device tables: every round's s(0) + s(1) is the running claim, the claim moves to
    s(r_j) (Lagrange, Python integers), every table is folded by r_j; at the end each table is one element, the form of
    these is the claim, and each is the original table's extension at (r_0, ..), reversed for HIGH"""
    import torch
    from sppark_amd import mle, poly
    m = _model(field)
    f = m.f
    lg = _T(field) + 3
    n = 1 << lg
    rows, vals, point = _case(field, lg)
    if form == M.PRODUCT:
        tables = [_dev(m, x) for x in rows[:3]]
        claim = m.full_sum(vals[:3], form)
    else:                                                       # e = eq(tau), a satisfied c = a .* b: the zero-check
        tau = _dev(m, point)
        e = torch.zeros_like(_dev(m, rows[0]))
        mle.eq(e, tau, field=field, stream=_stream())
        a, b = _dev(m, rows[1]), _dev(m, rows[2])
        c = torch.zeros_like(a)
        poly.vec_mul(c, a, b, field=field, stream=_stream())
        torch.cuda.synchronize()
        tables = [e, a, b, c]
        claim = m.zero
    originals = [t.clone() for t in tables]
    challenges = m.vals(m.random_rows(lg, 0xc4a11))
    size = n
    for j in range(lg):
        s = m.vals(mle.round([t[:size] for t in tables], form=form, order=order, field=field, stream=_stream()))
        assert m.add(s[0], s[1]) == claim, (field, form, order, j)
        claim = m.lagrange(s, challenges[j])
        r = f.shaped(m.rows([challenges[j]]))
        for k, t in enumerate(tables):
            if order == M.HIGH:
                view = t[:size]
                mle.fold(view, view, r, order=order, field=field, stream=_stream())
            else:
                out = torch.empty_like(t[:size // 2])
                mle.fold(out, t[:size], r, order=order, field=field, stream=_stream())
                tables[k] = out
        torch.cuda.synchronize()
        size //= 2
    finals = [m.vals(_back(m, t[:1]))[0] for t in tables]
    assert m.form(form, finals) == claim, (field, form, order)
    at = m.rows(challenges if order == M.LOW else challenges[::-1])
    for k, t in enumerate(originals):
        assert (mle.evaluate(t, f.shaped(at), field=field, stream=_stream()) == m.row(finals[k])).all(), (field, form, order, k)
