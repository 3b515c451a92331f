"""CPU: the route of an NTT call (sppark_amd/csrc/ntt/ntt_route.hpp make_ntt_route) against what the GPU ran.

tests/golden/ntt_launch_trace.json is the kernel trace of tools/gpu_ntt_launch_trace.py, recorded on an MI355X at the commit
BEFORE the driver followed a route: per case the call (field, entry point, size, mode, batch, stride, view offset, tuning
setting) and every dispatch of a transform kernel (name with template arguments, grid in work-items, work-group size, LDS
bytes).  Here the route is built from the recorded inputs -- by the same function and the same hooks the host emulation
runs its kernels over (tests/emu/emu_ntt.cpp) -- and must name exactly the recorded dispatches, with the recorded LDS size
wherever a step has dynamic LDS.  A cut-off that moves fails this test without a GPU.  What a trace cannot show (which
table a step reads, which one carries 1/n) is held by invariants at every size the entry points accept and in every mode,
and the shipped cut-offs themselves are pinned."""
import ctypes
import json
import os

import pytest

from test_emulation_ntt import FIELDS, _emu

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = os.path.join(HERE, "golden", "ntt_launch_trace.json")
WIDE = ("bls12_381", "bn254")
TWO_ADICITY = {"gl64": 32, "bb31": 27, "bls12_381": 32, "bn254": 28}
ELEM_BYTES = {"gl64": 8, "bb31": 4, "bls12_381": 32, "bn254": 32}
TILE_BITS = {"gl64": 5, "bb31": 6, "bls12_381": 4, "bn254": 4}          # bitrev_tile_bits<F>
# ntt_kernel, in the enum's order: (kernel template, the step fields that are its integer template arguments)
KERNELS = [("k_bitrev", ()), ("k_bitrev_tiled", ("TB",)), ("k_bitrev_tiled_vec", ("TB",)), ("k_coset", ()),
           ("k_ntt_small", ("inv", "LGC")), ("k_ntt_small_packed", ("inv", "LG")), ("k_ntt_pass", ("dif", "inv", "R1", "R2")),
           ("k_ntt_pass_lat", ("dif", "inv")), ("k_ntt6", ("dif", "inv")), ("k_ntt12", ("dif", "inv", "zero")),
           ("k_ntt12", ("zero", "zero", "one")), ("k_lde_spread", ()), (None, ())]
NK = {n: i for i, n in enumerate(["BITREV", "BITREV_TILED", "BITREV_TILED_VEC", "COSET", "SMALL", "SMALL_PACKED", "PASS", "PASS_LAT", "NTT6",
                                  "NTT12", "NTT12_LDE", "LDE_SPREAD", "COPY_OUT"])}
TRANSFORM = [NK[k] for k in ("SMALL", "SMALL_PACKED", "PASS", "PASS_LAT", "NTT6", "NTT12", "NTT12_LDE")]
HEAD = ("nsteps", "ntables", "overflow", "invalid", "cols", "gs", "inverse", "r64", "cmode", "lde_fused", "cap", "tcap", "launch_cols")
STEP = ("kernel", "R1", "R2", "LGC", "LG", "gx", "gy", "block", "lds", "p_lg_cur", "S", "lgC", "lgG", "apply_scale", "p_cmode", "lg_cur", "flags",
        "bitrev", "tw", "t1", "t2", "cz", "crow", "pass_tw", "lde_src", "lde_out", "stages", "scales")
TABLE = ("family", "kind", "lg_cur", "S", "cmode", "scaled", "count", "key_family", "key_a", "key_b", "key_c")
NT_PASS = 0
NL_NONE, NL_SPREAD, NL_OUT = 0, 1, 2


@pytest.fixture(scope="module")
def libs():
    return {field: _emu(feature) for field, feature in FIELDS}


def route(L, lg, order, direction, typ, batch=1, col_stride=0, max_grid_y=65535, aligned16=1, lde=NL_NONE, lg_domain=0, lg_blowup=0,
          no_r64=0, no_scaled_table=0):
    """(head, steps, tables) of make_ntt_route under the library's knobs; a table index of a step: 0 = none, else 1 + index"""
    call = (ctypes.c_uint * 13)(lg, order, direction, typ, batch, col_stride, max_grid_y, aligned16, lde, lg_domain, lg_blowup, no_r64, no_scaled_table)
    out = (ctypes.c_uint * 1024)()
    n = L.emu_ntt_route(call, out, 1024)
    assert n, "the route does not fit the buffer"
    head = dict(zip(HEAD, out[:len(HEAD)]))
    assert n == len(HEAD) + len(STEP) * head["nsteps"] + len(TABLE) * head["ntables"]
    o = len(HEAD)
    steps = [dict(zip(STEP, out[o + len(STEP) * i:o + len(STEP) * (i + 1)])) for i in range(head["nsteps"])]
    o += len(STEP) * head["nsteps"]
    tables = [dict(zip(TABLE, out[o + len(TABLE) * i:o + len(TABLE) * (i + 1)])) for i in range(head["ntables"])]
    assert not head["overflow"] and head["nsteps"] <= head["cap"] and head["ntables"] <= head["tcap"], (lg, order, direction, typ)
    return head, steps, tables


def _parse(name):
    """trace name `k_ntt_pass<fr256_dev<bls12_381_fr_p>, true, false, 2u, 1u>` -> ("k_ntt_pass", (1, 0, 2, 1)): without the field"""
    base, _, rest = name.partition("<")
    args, depth, cur = [], 0, ""
    for ch in rest.rstrip()[:-1]:
        if ch == "," and depth == 0:
            args.append(cur.strip()); cur = ""
            continue
        depth += ch == "<"
        depth -= ch == ">"
        cur += ch
    args.append(cur.strip())
    return base, tuple({"true": 1, "false": 0}.get(a, None) if a in ("true", "false") else int(a.rstrip("u")) for a in args[1:])


def _dispatches(field, head, steps):
    """what the profiler shows of a route: (kernel, template arguments, grid x and y in work-items, work-group size, dynamic LDS)"""
    out = []
    for s in steps:
        base, targs = KERNELS[s["kernel"]]
        if base is None:
            continue                                            # (a copy: no kernel of this library)
        v = dict(s, TB=TILE_BITS[field], dif=head["gs"], inv=head["inverse"], zero=0, one=1)
        out.append((base, tuple(v[a] for a in targs), s["gx"] * s["block"], s["gy"], s["block"], s["lds"]))
    return out


def _knobs(L, setting):
    """the tuning settings of tools/gpu_ntt_launch_trace.py SETTINGS, through the emulation's hooks"""
    wide = setting.get("wide", False)
    L.emu_ntt_plan(int(setting.get("SPPARK_NTT_R64_MIN", 12)), int(setting.get("SPPARK_NTT_R64_DIRECT", 20)))
    L.emu_ntt_coset_fold(int(setting.get("SPPARK_NTT_COSET_FOLD", 1)))
    L.emu_ntt_lat(int(setting.get("SPPARK_NTT_LAT_SMAX", 8 if wide else 0)), -1, -1)


def test_shipped_cut_offs(libs):
    """the defaults of ntt_knobs (ntt_route.hpp ntt_default_knobs), field by field: the values the measurements beside them chose"""
    for field, L in libs.items():
        out = (ctypes.c_uint * 14)()
        L.emu_ntt_knobs(out)
        wide = field in WIDE
        want = dict(smax=4 if wide else 8, lgc=5 if field == "bb31" else 4, lgt=10 if wide else 13 if field == "bb31" else 12, r64_min=12, r64_direct=20,
                    lat_smax=8 if wide else 0, lat_lgc=0, lat_lgt=0, coset_fold=1, small_max=9 if wide else 11, small_sized=1, packed_max=6,
                    wide_table_lg=24, pass_table_max_lg=16)
        assert dict(zip(want, out)) == want, field


def test_route_predicts_the_recorded_launches(libs):
    trace = json.load(open(TRACE))
    cols = trace["case_columns"]
    assert trace["columns"] == ["name", "grid_size_x", "grid_size_y", "workgroup_size_x", "group_segment_size"]
    names = [_parse(n) for n in trace["names"]]
    rows = trace["device"]["max_grid_y"]
    assert len(trace["cases"]) >= 1900
    nlds = 0
    try:
        for case in trace["cases"]:
            c = dict(zip(cols, case))
            field, lg = c["field"], c["lg"]
            L = libs[field]
            _knobs(L, dict(trace["settings"][c["setting"]], wide=field in WIDE))
            eb = ELEM_BYTES[field]
            if c["kind"] == 2:                                  # sppark_lde[_batch]: iNTT(NR) handing its result over, NTT(RN) taking the compact source
                lgd, lgb = lg, c["order"]
                ext = 1 << (lgd + lgb)
                h1, s1, _ = route(L, lgd, 1, 1, 0, batch=c["batch"], col_stride=ext, max_grid_y=rows, lde=NL_OUT)
                h2, s2, _ = route(L, lgd + lgb, 2, 0, 0, batch=c["batch"], col_stride=ext, max_grid_y=rows, lde=NL_SPREAD, lg_domain=lgd, lg_blowup=lgb)
                assert h1["cols"] == h2["cols"] == c["batch"]
                want = _dispatches(field, h1, s1) + _dispatches(field, h2, s2)
                # (the spread: separate buffers, one launch over every output element -- ntt_engine::lde_spread)
                want = [(k, t, -(-ext // 256) * 256 if k == "k_lde_spread" else gx, gy, 256 if k == "k_lde_spread" else b, l) for k, t, gx, gy, b, l in want]
            else:
                stride = c["stride"] or (1 << lg)
                aligned = (c["offset"] * eb) % 16 == 0 and (c["batch"] == 1 or (stride * eb) % 16 == 0)
                h, s, _ = route(L, lg, c["order"], c["direction"], c["type"], batch=c["batch"], col_stride=stride, max_grid_y=rows, aligned16=int(aligned))
                assert h["cols"] == c["batch"] and not h["invalid"], case
                want = _dispatches(field, h, s)
            got = [names[d[0]] + tuple(d[1:4]) for d in c["dispatches"]]
            assert got == [w[:5] for w in want], (case, want)
            # dynamic LDS: the kernels that take any have no static LDS, so the recorded segment is the route's figure
            for w, d in zip(want, c["dispatches"]):
                assert w[5] == 0 or w[5] == d[4], (case, w)
            nlds += sum(1 for w in want if w[5])
    finally:
        for field, L in libs.items():
            _knobs(L, dict(wide=field in WIDE))
    assert nlds > 3000


MODES = [(o, d, t) for o in range(4) for d in range(2) for t in range(2)]


def _check(field, lg, order, direction, typ, head, steps, tables, lde=NL_NONE, no_scaled_table=0, no_r64=0):
    what = (field, lg, order, direction, typ, lde)
    assert not head["invalid"], what
    kinds = [s["kernel"] for s in steps]
    # the stages of the steps add up to lg
    assert sum(s["stages"] for s in steps) == lg, what
    assert all((s["stages"] != 0) == (s["kernel"] in TRANSFORM) for s in steps), what
    # 1/n: by exactly one step of an inverse transform -- itself or through the one scaled table --, by none of a forward one
    by_table = [s for s in steps if any(s[r] and tables[s[r] - 1]["scaled"] for r in ("tw", "t1", "t2", "pass_tw"))]
    by_step = [s for s in steps if s["apply_scale"] or (s["kernel"] in (NK["SMALL"], NK["SMALL_PACKED"]) and head["inverse"])]
    assert len(by_table) + len(by_step) == direction == sum(s["scales"] for s in steps), what
    assert sum(t["scaled"] for t in tables) == len(by_table), what
    # ... carried by the table of the tabled pass on the SMALLEST sub-problems where the plan has one (the radix-64 plan: its last step's)
    passes = [t for t in tables if t["family"] == NT_PASS]
    if direction and passes and not head["r64"] and not no_scaled_table:
        assert [t["lg_cur"] for t in passes if t["scaled"]] == [min(t["lg_cur"] for t in passes)], what
    if direction and head["r64"]:
        last = [s for s in steps if s["kernel"] in TRANSFORM][-1]
        assert (by_step if last["kernel"] == NK["PASS"] else by_table) == [last], what
    # every table a step names exists, and every requested table but the 64 coset constants is read
    used = {s[r] - 1 for s in steps for r in ("tw", "t1", "t2", "cz", "crow", "pass_tw") if s[r]}
    assert used <= set(range(len(tables))) and set(range(len(tables))) - used <= {i for i, t in enumerate(tables) if t["family"] == 2}, what
    # a coset transform: folded (no k_coset) or exactly one k_coset, in front of a forward and behind an inverse transform,
    # with the exponents of the order the data is in there (NN: behind its bit reversal; RR: in front of it)
    ncoset = kinds.count(NK["COSET"])
    small = any(k in (NK["SMALL"], NK["SMALL_PACKED"]) for k in kinds)
    if typ == 0 or head["cmode"] or small:
        assert ncoset == 0, what
        assert not head["cmode"] or (typ == 1 and order != 3 and head["r64"]), what
    else:
        assert ncoset == 1, what
        i = kinds.index(NK["COSET"])
        first = min(j for j, k in enumerate(kinds) if k in TRANSFORM)
        last = max(j for j, k in enumerate(kinds) if k in TRANSFORM)
        if direction == 0:
            assert i < first and steps[i]["bitrev"] == int(order != 1), what        # (only NR has its input in natural order there)
            assert order != 0 or kinds[0] in (NK["BITREV"], NK["BITREV_TILED"], NK["BITREV_TILED_VEC"]) and i == 1, what
        else:
            assert i > last and steps[i]["bitrev"] == int(order == 1), what         # (only NR has its output bit-reversed there)
            assert order != 3 or i == len(steps) - 2, what
    # the LDE's hand-over is consumed exactly once
    assert sum(s["lde_src"] for s in steps) == (lde == NL_SPREAD) and sum(s["lde_out"] for s in steps) == (lde == NL_OUT), what
    assert head["lde_fused"] == (NK["NTT12_LDE"] in kinds), what


def test_route_invariants_at_every_size_and_mode(libs):
    for field, L in libs.items():
        for lg in range(0, TWO_ADICITY[field] + 1):
            for order, direction, typ in MODES:
                h, s, t = route(L, lg, order, direction, typ)
                if lg == 0:
                    assert h["nsteps"] == 0
                    continue
                _check(field, lg, order, direction, typ, h, s, t)
            # sppark_lde's two transforms, every blow-up
            h, s, t = route(L, lg, 1, 1, 0, lde=NL_OUT)
            if lg:
                _check(field, lg, 1, 1, 0, h, s, t, NL_OUT)
            assert sum(x["lde_out"] for x in s) == 1
            for lgb in range(0, min(lg, 5) + 1):
                h, s, t = route(L, lg, 2, 0, 0, lde=NL_SPREAD, lg_domain=lg - lgb, lg_blowup=lgb)
                if lg:
                    _check(field, lg, 2, 0, 0, h, s, t, NL_SPREAD)
                assert sum(x["lde_src"] for x in s) == 1
            # the refusals: no step of the radix-64 plan / no scaled table, and the invariants hold
            if lg:
                for refuse in (dict(no_r64=1), dict(no_scaled_table=1), dict(no_r64=1, no_scaled_table=1)):
                    h, s, t = route(L, lg, 1, 1, 1, **refuse)
                    _check(field, lg, 1, 1, 1, h, s, t, **refuse)
                    if "no_r64" in refuse:
                        assert not h["r64"] and not any(x["kernel"] in (NK["NTT6"], NK["NTT12"]) for x in s)
                    if len(refuse) == 2 or (not h["r64"] and "no_scaled_table" in refuse):
                        assert not any(x["scaled"] for x in t)
        assert route(L, TWO_ADICITY[field] + 1, 1, 0, 0)[0]["invalid"] and route(L, 8, 4, 0, 0)[0]["invalid"]


def test_batches_split_into_launch_chunks(libs):
    """A batch above what one launch can index runs as chunks, each with its own route: with a grid of at most 4 rows the
    chunks cover every column exactly once; the packed kernel takes 4 << (9 - lg) columns per chunk, a work-group of
    256 lanes 512 >> lg of them."""
    for field, L in libs.items():
        for lg, batch in ((3, 9), (8, 9), (3, 600), (6, 33), (7, 5)):
            packed = lg <= 6
            done = 0
            while done < batch:
                h, s, _ = route(L, lg, 1, 0, 0, batch=batch - done, col_stride=1 << lg, max_grid_y=4)
                assert h["launch_cols"] == (4 << (9 - lg) if packed else 4), (field, lg)
                assert h["cols"] == min(batch - done, h["launch_cols"]) and h["nsteps"] == 1
                if s[0]["kernel"] == NK["SMALL_PACKED"]:
                    per = 512 >> lg
                    assert packed and h["cols"] > 1 and s[0]["LG"] == lg and (s[0]["gy"] - 1) * per < h["cols"] <= s[0]["gy"] * per <= 4 * per
                else:
                    assert s[0]["kernel"] == NK["SMALL"] and s[0]["gy"] == h["cols"] <= 4 and (not packed or h["cols"] == 1)
                done += h["cols"]
            assert done == batch
