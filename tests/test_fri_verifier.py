"""CPU: the teeth of tests/fri_verifier.py.  A slow honest prover in Python integers (tests/fri_model.py does the folding: it
is the thing being cross-examined) over 2^6 points, blow-up 4, must be accepted for every field pair in both orders, and each
single corruption of its transcript must be rejected with the check named here.  This is what makes an "accept" of the
device prover (tests/test_fri_protocol_gpu.py) mean something."""
import copy
import functools

import pytest

import fri_model as FM
import fri_verifier as V
import merkle_model as MM

LG_N, LG_BLOWUP = 6, 2
K = LG_N - LG_BLOWUP
FULL, EARLY = (1, 2, 1), (3,)                               # sum = K: a constant is left; early stop: degree below 2 on 8 points
PAIRS = [("gl64", "gl64"), ("bb31", "bb31x4"), ("bls12_381", "bls12_381")]
ORDERS = [V.NATURAL, V.BITREV]
WIDTHS = (5, 3)


@functools.lru_cache(maxsize=None)
def _model(field):
    return FM.FriModel(field)


def _inv(m, e):
    """1 / e; in the quartic extension e^(p^4 - 2)"""
    if not m.x4:
        return pow(e, -1, m.p)
    r, sq, k = m.one, e, m.p ** 4 - 2
    while k:
        if k & 1:
            r = m.mul(r, sq)
        sq, k = m.mul(sq, sq), k >> 1
    assert m.mul(r, e) == m.one
    return r


def _groups(code, a, order):
    """the fold groups as the 2-D views of the device prover have them: BITREV (n / A, A) by rows, NATURAL (A, n / A) by columns"""
    A, n = 1 << a, len(code)
    if order == V.BITREV:
        return [code[j * A:(j + 1) * A] for j in range(n // A)]
    return [code[j::n // A] for j in range(n // A)]


def prove(trace_field, field, order, arities, cheat=None, hash_="blake2s", seed=1):
    m, tm = _model(field), _model(trace_field)
    lifted = trace_field != field
    lift = (lambda c: m.embed(c)) if lifted else (lambda c: c)
    n = 1 << LG_N
    t = dict(trace_field=trace_field, field=field, hash=hash_, order=order, lg_n=LG_N, lg_blowup=LG_BLOWUP, arities=list(arities),
             widths=list(WIDTHS), forced=[0, n - 1], layer_roots=[])
    xs = m.domain(LG_N, "coset", order)
    coeffs = [tm.vals(tm.random_rows(1 << K, 100 * seed + j)) for j in range(sum(WIDTHS))]
    coeffs[0][1], coeffs[1][2], coeffs[5][0] = 0, 1, tm.p - 1
    evals = [tm.evaluate_poly(c, xs) for c in coeffs]
    mats = [evals[:WIDTHS[0]], evals[WIDTHS[0]:]]
    trace_leaves = [[V.to_bytes(tm, [col[i] for col in mat]) for i in range(n)] for mat in mats]
    trace_trees = [MM.layers(leaves, hash_) for leaves in trace_leaves]
    t["trace_roots"] = [tree[-1][0] for tree in trace_trees]
    fs = V.FiatShamir(t)
    z = fs.z()
    assert fs.z_draws == 1                                              # the first draw lies outside both domains
    t["z"] = V.to_bytes(m, [z])
    v = []
    for c in coeffs:                                                    # Horner in the codeword field
        acc = m.zero
        for x in reversed(c):
            acc = m.add(m.mul(acc, z), lift(x))
        v.append(acc)
    if cheat == "opening":
        v[3] = m.add(v[3], m.one)
    t["openings"] = [V.to_bytes(m, [x]) for x in v]
    alpha = fs.alpha()
    apow = [m.one]
    for _ in range(len(v) - 1):
        apow.append(m.mul(apow[-1], alpha))
    claimed = m.total(m.mul(a, x) for a, x in zip(apow, v))
    code = []
    for i in range(n):
        num = m.sub(m.total(m.mul(a, lift(col[i])) for a, col in zip(apow, evals)), claimed)
        code.append(m.mul(num, _inv(m, m.sub(m.embed(xs[i]), z))))
    shift, layers = m.coset_shift(), []
    for r, a in enumerate(arities):
        groups = _groups(code, a, V.NATURAL if cheat == "natural_groups" else order)
        leaves = [V.to_bytes(m, grp) for grp in groups]
        tree = MM.layers(leaves, hash_)
        layers.append((leaves, tree))
        t["layer_roots"].append(tree[-1][0])
        beta = fs.beta(r)
        if cheat == "beta" and r == 1:
            beta = m.add(beta, m.one)
        used = shift
        if cheat == "shift" and r == 1:
            used = m.coset_shift()                                      # not raised to 2^a_0
        code = m.fold(code, a, beta, used, order)
        shift = pow(shift, 1 << a, m.p)
    if cheat == "random_final":
        code = m.vals(m.random_rows(len(code), 77))
    if cheat == "final_entry":
        code[1] = m.add(code[1], m.one)
    t["final"] = V.to_bytes(m, code)
    t["queries"] = []
    for i in fs.indices():
        q = {"trace": [(leaves[i], MM.path(tree, i)) for leaves, tree in zip(trace_leaves, trace_trees)], "layers": []}
        at, lg = i, LG_N
        for (leaves, tree), a in zip(layers, arities):
            at = at >> a if order == V.BITREV else at % (1 << (lg - a))
            q["layers"].append((leaves[at], MM.path(tree, at)))
            lg -= a
        t["queries"].append(q)
    return t


@functools.lru_cache(maxsize=None)
def _honest(trace_field, field, order, arities):
    return prove(trace_field, field, order, arities)


def _indices(t):
    fs = V.FiatShamir(t)
    fs.z(), fs.alpha(), [fs.beta(r) for r in range(len(t["arities"]))]
    return fs.indices()


def _flip(data, at=0):
    data = bytearray(data)
    data[at] ^= 1
    return bytes(data)


HONEST = [(tf, f, o, a, "blake2s") for tf, f in PAIRS for o in ORDERS for a in (FULL, EARLY)] + [("gl64", "gl64", o, FULL, "sha256") for o in ORDERS]


@pytest.mark.parametrize("trace_field,field,order,arities,hash_", HONEST)
def test_honest_transcript_is_accepted(oracle, trace_field, field, order, arities, hash_):
    t = _honest(trace_field, field, order, arities) if hash_ == "blake2s" else prove(trace_field, field, order, arities, hash_=hash_)
    assert V.verify(t) is None
    # handed the same challenges, it accepts as well; handed another beta, it does not
    fs = V.FiatShamir(t)
    ch = dict(z=fs.z(), alpha=fs.alpha(), betas=[fs.beta(r) for r in range(len(arities))], indices=fs.indices())
    assert V.verify(t, ch) is None
    m = _model(field)
    ch["betas"][-1] = m.add(ch["betas"][-1], m.one)
    assert V.verify(t, ch) == "fold"


# corruptions of a finished transcript: (name, what it does to a copy, the check that must fail)
def _trace_leaf(t):
    leaf, path = t["queries"][3]["trace"][1]
    t["queries"][3]["trace"][1] = (_flip(leaf, 5), path)


def _opening(t):
    t["openings"][6] = _flip(t["openings"][6])


def _member(t):
    leaf, path = t["queries"][2]["layers"][1]
    t["queries"][2]["layers"][1] = (_flip(leaf, len(leaf) - 1), path)


AFTER = [("trace_leaf", _trace_leaf, "trace_path"),
         ("opening", _opening, "deep"),             # alpha and all later challenges move; the forced index 0 is still asked first
         ("member", _member, "layer_path")]
# corruptions while proving, the prover honest from there on: (cheat, the check that must fail)
DURING = [("opening", "final"),                     # a consistent quotient of the wrong claim is no polynomial: every query holds
          ("beta", "fold"),
          ("shift", "fold"),
          ("random_final", "fold")]                 # query 0 ends in the final layer's entry 0


@pytest.mark.parametrize("name,corrupt,check", AFTER, ids=[c[0] for c in AFTER])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("trace_field,field", PAIRS)
def test_corrupted_transcript_is_rejected(oracle, trace_field, field, order, name, corrupt, check):
    t = copy.deepcopy(_honest(trace_field, field, order, FULL))
    corrupt(t)
    assert V.verify(t) == check


@pytest.mark.parametrize("cheat,check", DURING, ids=[c[0] for c in DURING])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("trace_field,field", PAIRS)
def test_cheating_prover_is_rejected(oracle, trace_field, field, order, cheat, check):
    assert V.verify(prove(trace_field, field, order, FULL, cheat=cheat)) == check


@pytest.mark.parametrize("trace_field,field", PAIRS)
def test_natural_groups_for_a_bitrev_transcript_are_rejected(oracle, trace_field, field):
    """the prover commits and serves the groups n / A apart although the codeword is bit-reversed: every path verifies, the
    followed value of query 0 is the same element, and the fold of what the leaf holds is not the next layer's value"""
    assert V.verify(prove(trace_field, field, V.BITREV, FULL, cheat="natural_groups")) == "fold"


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("trace_field,field", PAIRS)
def test_one_wrong_entry_of_the_final_layer_is_rejected(oracle, trace_field, field, order):
    """by the fold of the first query that ends in that entry; by the final check when no query does"""
    t = prove(trace_field, field, order, FULL, cheat="final_entry")
    ends = []
    for i in _indices(t):
        lg = LG_N
        for a in FULL:
            i, lg = (i >> a if order == V.BITREV else i % (1 << (lg - a))), lg - a
        ends.append(i)
    assert V.verify(t) == ("fold" if 1 in ends else "final")


@pytest.mark.parametrize("arities", [FULL, EARLY])
@pytest.mark.parametrize("order", ORDERS)
def test_wrong_opening_with_an_early_stop(oracle, order, arities):
    assert V.verify(prove("bb31", "bb31x4", order, arities, cheat="opening")) == "final"


@pytest.mark.parametrize("field", ["gl64", "bb31x4"])
@pytest.mark.parametrize("order", ORDERS)
def test_final_check_is_a_degree_bound(oracle, field, order):
    m = _model(field)
    lg = 3
    w = V.root_of_unity(m.base_field, lg)
    xs = m.domain(lg, 12345, order)
    for d in (1, 2, 4):
        c = m.vals(m.random_rows(d + 1, 31 + d))
        assert V.final_check(m, m.evaluate_poly(c[:d], xs), d, w, order, lg)
        assert not V.final_check(m, m.evaluate_poly(c, xs), d, w, order, lg)            # degree d
    assert not V.final_check(m, m.vals(m.random_rows(8, 9)), 4, w, order, lg)


def test_z_inside_a_domain_is_redrawn(oracle):
    m = _model("gl64")
    g = m.coset_shift()
    w = V.root_of_unity("gl64", LG_N)
    assert not V.outside(m, g * pow(w, 5, m.p) % m.p, g, LG_N, LG_BLOWUP)           # on the evaluation domain
    assert not V.outside(m, pow(w, 4 * 3, m.p), g, LG_N, LG_BLOWUP)                 # on the trace domain
    assert V.outside(m, 12345, g, LG_N, LG_BLOWUP)
    x = _model("bb31x4")
    gb = x.coset_shift()
    assert not V.outside(x, (gb, 0, 0, 0), gb, LG_N, LG_BLOWUP) and V.outside(x, (gb, 1, 0, 0), gb, LG_N, LG_BLOWUP)
    t = copy.deepcopy(_honest("gl64", "gl64", V.NATURAL, FULL))
    t["z"] = V.to_bytes(m, [g])
    assert V.verify(t) == "z"
