"""GPU: a whole FRI / DEEP prover on device tensors through the public Python API -- LDE_batch / compute_ntt_batch,
merkle.commit / open / gather, poly.evaluate / divide, fri.reduce / domain / fold / deep_quotient -- judged by the pure-Python
verifier of tests/fri_verifier.py (whose teeth tests/test_fri_verifier.py shows on the CPU).  Values reach the host only as
opened leaves, paths, roots, the claimed openings and the final layer.  Every comparison is exact.

What the accept establishes between the modules: the coset and order the transforms leave a matrix on are the shift="coset"
and order of fri.domain and fri.fold; the leaf of a FRI layer is one fold group, a 2-D view of the codeword -- BITREV
(n / A, A) with layout "rows", NATURAL (A, n / A) with layout "columns" -- and its leaf index is the index of the folded
value; the folded domain has the shift shift^A; a BabyBear trace is combined under bb31x4 challenges with base=True;
accumulate continues one power sequence over a second matrix; the aux_out coefficients feed poly.evaluate on the device.

Shapes: the first codeword has 2^(T + 1) elements (two tiles of csrc/fri/fri_route.hpp), blow-up 4."""
import functools

import numpy as np
import pytest

import fri_model as FM
import fri_verifier as V
from test_fri_gpu import _T, _dev, _host

pytestmark = pytest.mark.gpu

LG_BLOWUP = 2
WIDTHS = (5, 3)
# (trace field, codeword field): lg_n = T + 1 = 12 / 11 / 10 / 13, k = lg_n - 2; each schedule uses every arity and sums to k
SCHEDULE = {("gl64", "gl64"): (3, 3, 3, 1), ("bb31", "bb31x4"): (3, 3, 2, 1), ("bls12_381", "bls12_381"): (3, 2, 2, 1),
            ("bb31", "bb31"): (3, 3, 2, 2, 1)}
PAIRS = list(SCHEDULE)


@functools.lru_cache(maxsize=None)
def _model(field):
    return FM.FriModel(field)


def _bytes(x):
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).tobytes()


def _elem(m, val):
    """one element as the host argument the calls take"""
    return m.f.shaped(m.rows([val]))


def _trace(tm, width, k, seed):
    """width rows of 2^k canonical evaluations with 0, 1 and p - 1 planted (as test_fri_gpu._case plants them)"""
    n = 1 << k
    x = tm.random_rows(width * n, seed).reshape(width, n, tm.f.w)
    for j, edge in enumerate((0, tm.f.one, tm.f.pm1)):
        x[j % width, (3 * j + 1) % n] = edge
    return x


def _predrawn(m, lg_n, arities, seed):
    """challenges drawn before the prover runs: a z outside both domains, alpha, one beta per layer, 12 query indices"""
    g = m.coset_shift()
    zs = [z for z in m.vals(m.random_rows(4, seed)) if V.outside(m, z, g, lg_n, LG_BLOWUP)]
    rest = m.vals(m.random_rows(1 + len(arities), seed + 1))
    idx = np.random.default_rng(seed + 2).integers(0, 1 << lg_n, size=V.DRAWN_QUERIES)
    return dict(z=zs[0], alpha=rest[0], betas=rest[1:], drawn=[int(i) for i in idx])


def _prove(trace_field, field, order, arities, hash_="blake2s", mode="plain", negative=None):
    """The device prover.  mode: "plain"; "deep_quotient" (one matrix of width 8 through fri.deep_quotient); "stream" (all
    challenges drawn in advance, everything enqueued on one non-default stream without a synchronize() of the test's own,
    NATURAL folds in place).  negative: None, "trace", "opening" or "shift".  Returns (transcript, challenges or None, what the
    Horner check needs)."""
    import torch
    import sppark_amd as S
    from sppark_amd import fri, merkle, poly
    m, tm = _model(field), _model(trace_field)
    f, tf = m.f, tm.f
    lifted = trace_field != field
    lg_n = _T(m) + 1
    k, n = lg_n - LG_BLOWUP, 1 << lg_n
    assert sum(arities) <= k
    widths = (sum(WIDTHS),) if mode == "deep_quotient" else WIDTHS
    inplace = mode == "stream" and order == fri.NATURAL
    a0 = arities[0]
    edge = 1 << (_T(m) - a0)                                # layer-1 indices edge - 1, edge: last group of tile 0, first of tile 1
    forced = [0, n - 1] + [(j << a0) if order == fri.BITREV else j for j in (edge - 1, edge)]
    t = dict(trace_field=trace_field, field=field, hash=hash_, order=order, lg_n=lg_n, lg_blowup=LG_BLOWUP, arities=list(arities),
             widths=list(widths), forced=forced, trace_roots=[], layer_roots=[])
    ch = _predrawn(m, lg_n, arities, 0xf21) if mode == "stream" else None
    fs = None if ch else V.FiatShamir(t)
    g = m.base.vals(np.frombuffer(fri.coset_shift(field).tobytes(), dtype=m.base.f.dtype).reshape(1, -1))[0]     # (once, beforehand)
    stream = torch.cuda.Stream() if ch else torch.cuda.current_stream()
    s = stream.cuda_stream
    with torch.cuda.stream(stream):
        # ---- the trace: evaluations -> coefficients and the codeword matrices, committed where the transform left them ----
        mats, coeffs, trees = [], [], []
        for which, width in enumerate(widths):
            ev = _dev(_trace(tm, width, k, 700 + which).reshape(width, -1))
            ext = torch.zeros((width, n * tf.w), dtype=ev.dtype, device="cuda")
            ext[:, :ev.shape[1]] = ev
            co = torch.zeros_like(ev)
            S.LDE_batch(0, ext, k, LG_BLOWUP, field=trace_field, aux_out=co, stream=s)
            if order == fri.BITREV:
                ext = torch.zeros_like(ext)
                ext[:, :co.shape[1]] = co
                S.compute_ntt_batch(0, ext, S.NTTInputOutputOrder.NR, S.NTTDirection.Forward, S.NTTType.Coset, field=trace_field, stream=s)
            tree, root = merkle.commit(ext, hash=hash_, layout="columns", field=trace_field, stream=s)
            mats.append(ext); coeffs.append(co); trees.append((tree, root))
        if fs:
            t["trace_roots"] = [_bytes(root) for _tree, root in trees]
            z = fs.z()
        else:
            z = ch["z"]
        t["z"] = V.to_bytes(m, [z])
        d_z = _dev(m.rows([z]))

        # ---- the openings: poly.evaluate on the device coefficient rows ----
        nv = sum(widths)
        d_v = torch.zeros((nv, f.w), dtype=d_z.dtype, device="cuda")
        rows = [co[j] for co in coeffs for j in range(co.shape[0])]
        if lifted:                                                      # into component 0 of the extension, on the device
            up = torch.zeros((nv, 1 << k, 4), dtype=d_z.dtype, device="cuda")
            up[:, :, 0] = torch.stack(rows)
            rows = [up[j].reshape(-1) for j in range(nv)]
        for j, row in enumerate(rows):
            poly.evaluate(d_v[j], d_z.reshape(-1), row, field=field, stream=s)
        if negative == "opening":
            d_v[3] = d_v[4]
        if fs:
            t["openings"] = [_bytes(d_v[j]) for j in range(nv)]
            alpha = fs.alpha()
        else:
            alpha = ch["alpha"]
        apow = [m.one]
        for _ in range(nv - 1):
            apow.append(m.mul(apow[-1], alpha))
        d_w = _dev(m.rows(apow))
        if fs:                                                          # sum_j alpha^j v_j, a host element
            sub = _elem(m, m.total(m.mul(a, v) for a, v in zip(apow, V.from_bytes(m, b"".join(t["openings"])))))
        else:                                                           # nothing may come back yet: the same sum as a one-leaf reduce
            sub = torch.zeros((1, f.w), dtype=d_z.dtype, device="cuda")
            fri.reduce(sub, d_v, d_w, layout="columns", field=field, stream=s)

        # ---- DEEP: (sum_j alpha^j f_j - sum_j alpha^j v_j) / (x - z) ----
        code = torch.zeros((n, f.w), dtype=d_z.dtype, device="cuda")
        if negative == "trace":                                         # one element differs while reduce reads it, at the forced index n - 1
            at = slice((n - 1) * tf.w, n * tf.w)
            saved = mats[0][2, at].clone()
            mats[0][2, at] = mats[0][2, :tf.w]
        if mode == "deep_quotient":
            fri.deep_quotient(code, mats[0], d_w, sub, d_z, lg_n=lg_n, shift="coset", order=order, layout="columns", base=lifted,
                              field=field, stream=s)
        else:
            den = torch.zeros_like(code)
            fri.reduce(code, mats[0], d_w[:WIDTHS[0]], sub=sub, layout="columns", base=lifted, field=field, stream=s)
            fri.reduce(code, mats[1], d_w[WIDTHS[0]:], accumulate=True, layout="columns", base=lifted, field=field, stream=s)
            fri.domain(den, shift="coset", order=order, z=d_z, field=field, stream=s)
            poly.divide(code, code, den, field=field, stream=s)
        if negative == "trace":
            mats[0][2, at] = saved

        # ---- the commit phase: the leaf of a layer is one fold group ----
        def layer_indices(idx):
            """per layer, the leaf index of every query's group"""
            out, at, lg = [], np.array(idx, dtype=np.int64), lg_n
            for a in arities:
                at = at >> a if order == fri.BITREV else at % (1 << (lg - a))
                out.append(at.copy())
                lg -= a
            return out
        early = layer_indices(forced + ch["drawn"]) if ch else None     # in place: a layer's leaves go before its fold overwrites them
        layers, leaves, shift = [], [], g
        for r, a in enumerate(arities):
            A, n_r = 1 << a, code.shape[0]
            if order == fri.BITREV:
                view, layout = code.reshape(n_r // A, A * f.w), "rows"
            else:
                view, layout = code.reshape(A, (n_r // A) * f.w), "columns"
            tree, root = merkle.commit(view, hash=hash_, layout=layout, field=field, stream=s)
            layers.append((view, layout, tree, root))
            if fs:
                t["layer_roots"].append(_bytes(root))
                beta = fs.beta(r)
            else:
                beta = ch["betas"][r]
                leaves.append(merkle.gather(view, early[r], layout=layout, field=field, stream=s))
            sh = "coset" if r == 0 else m.base.f.shaped(m.base.rows([shift]))
            if negative == "shift" and r == 1:
                sh = None
            if inplace:
                fri.fold(code, code, _elem(m, beta), lg_arity=a, shift=sh, order=order, field=field, stream=s)
                code = code[:n_r // A]
            else:
                out = torch.zeros((n_r // A, f.w), dtype=code.dtype, device="cuda")
                fri.fold(out, code, _elem(m, beta), lg_arity=a, shift=sh, order=order, field=field, stream=s)
                code = out
            shift = pow(shift, A, m.p)
        if fs:
            t["final"] = _bytes(code)
            idx = fs.indices()
        else:
            idx = forced + ch["drawn"]

        # ---- the queries ----
        opened = []
        for (tree, _root), ext in zip(trees, mats):
            opened.append((merkle.gather(ext, idx, layout="columns", field=trace_field, stream=s),
                           merkle.open(tree, lg_n, idx, field=trace_field, stream=s)))
        per_layer = layer_indices(idx)
        lg = lg_n
        for r, ((view, layout, tree, _root), a) in enumerate(zip(layers, arities)):
            lg -= a
            got = leaves[r] if ch else merkle.gather(view, per_layer[r], layout=layout, field=field, stream=s)
            opened.append((got, merkle.open(tree, lg, per_layer[r], field=field, stream=s)))
    if ch:
        stream.synchronize()                                            # the one synchronisation
        t["trace_roots"] = [_bytes(root) for _tree, root in trees]
        t["openings"] = [_bytes(d_v[j]) for j in range(nv)]
        t["layer_roots"] = [_bytes(root) for _v, _l, _t, root in layers]
        t["final"] = _bytes(code)
        ch = dict(z=ch["z"], alpha=ch["alpha"], betas=ch["betas"], indices=idx)
    opened = [(rows_.cpu().numpy(), paths.cpu().numpy()) for rows_, paths in opened]
    t["queries"] = []
    for q in range(len(idx)):
        pairs = [(rows_[q].tobytes(), [p.tobytes() for p in paths[q]]) for rows_, paths in opened]
        t["queries"].append({"trace": pairs[:len(widths)], "layers": pairs[len(widths):]})
    return t, ch, (coeffs, z)


def _check_openings(t, coeffs, z):
    """the claimed openings against Horner in Python integers over the coefficients read back"""
    m, tm = _model(t["field"]), _model(t["trace_field"])
    lift = m.embed if t["trace_field"] != t["field"] else (lambda c: c)
    v = V.from_bytes(m, b"".join(t["openings"]))
    j = 0
    for co in coeffs:
        for row in _host(co, tm).reshape(co.shape[0], -1, tm.f.w):
            acc = m.zero
            for c in reversed(tm.vals(row)):
                acc = m.add(m.mul(acc, z), lift(c))
            assert acc == v[j], (t["field"], j)
            j += 1


CASES = [(tf, f, order, SCHEDULE[tf, f], "blake2s", "plain") for tf, f in PAIRS for order in (V.NATURAL, V.BITREV)] + [
    ("gl64", "gl64", V.NATURAL, (3, 3, 3), "blake2s", "plain"),                         # early stop: degree below 2 on 8 points
    ("gl64", "gl64", V.BITREV, (3, 3, 3), "blake2s", "plain"),
    ("gl64", "gl64", V.NATURAL, SCHEDULE["gl64", "gl64"], "sha256", "plain"),
    ("gl64", "gl64", V.BITREV, SCHEDULE["gl64", "gl64"], "sha256", "plain"),
    ("bb31", "bb31x4", V.NATURAL, SCHEDULE["bb31", "bb31x4"], "blake2s", "deep_quotient"),
    ("bls12_381", "bls12_381", V.BITREV, SCHEDULE["bls12_381", "bls12_381"], "blake2s", "deep_quotient"),
    ("gl64", "gl64", V.NATURAL, SCHEDULE["gl64", "gl64"], "blake2s", "stream"),          # in place
    ("bb31", "bb31x4", V.NATURAL, SCHEDULE["bb31", "bb31x4"], "blake2s", "stream"),      # in place
    ("bb31", "bb31x4", V.BITREV, SCHEDULE["bb31", "bb31x4"], "blake2s", "stream"),
]


def _id(c):
    return "-".join([c[0], c[1], "bitrev" if c[2] else "natural", "".join(map(str, c[3])), c[4], c[5]])


@pytest.mark.parametrize("trace_field,field,order,arities,hash_,mode", CASES, ids=[_id(c) for c in CASES])
def test_device_prover_is_accepted(oracle, libs, trace_field, field, order, arities, hash_, mode):
    t, ch, (coeffs, z) = _prove(trace_field, field, order, arities, hash_, mode)
    assert V.verify(t, ch) is None
    _check_openings(t, coeffs, z)


NEGATIVE = [("trace", "deep"),        # reduce read a matrix that differs from the committed one at the forced index n - 1
            ("opening", "final"),     # a consistent quotient of a wrong claim is no polynomial
            ("shift", "fold")]        # layer 1 folded over the domain without its shift


@pytest.mark.parametrize("negative,check", NEGATIVE, ids=[c[0] for c in NEGATIVE])
@pytest.mark.parametrize("order", [V.NATURAL, V.BITREV])
def test_device_side_negative_controls_are_rejected(oracle, libs, order, negative, check):
    """host-side argument changes only; each must make the verifier reject, with the check that sees it"""
    t, ch, _ = _prove("gl64", "gl64", order, SCHEDULE["gl64", "gl64"], negative=negative)
    assert V.verify(t, ch) == check
