"""CPU: the route of an MSM (sppark_amd/csrc/msm/msm_route.hpp) against what the GPU ran.

tests/golden/msm_launch_trace.json is the kernel trace of tools/gpu_msm_launch_trace.py, recorded on an MI355X at the
commit BEFORE the driver followed a route: per case the inputs, the plan the context reported and every dispatch (kernel
with template arguments, grid in work-items, work-group size, LDS bytes).  Here the plan is rebuilt from the recorded
inputs, must equal the recorded one -- which pins the resident-lane count the device reported -- and the route must name
exactly the recorded dispatches from the point conversion / accumulation to the end of the invoke, the second pass of
the all-equal-scalar cases included, with the recorded LDS size wherever a step has dynamic LDS.  A threshold that moves
fails this test without a GPU.  Two kinds of case have no recorded plan of their own and are pinned through their grids
alone: G2 (the entry point's contexts are pooled and report no plan) and the fixed-base case (the context reports the
ordinary plan of its size, not the one-window plan that ran).  Also: the decoder of sppark_msm_tune_tail's numeric code."""
import ctypes
import json
import os
import re

import pytest

from test_plan import FIELD_G1, KEYS, check_route, plan_lib, plan_tuned, route          # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = os.path.join(HERE, "golden", "msm_launch_trace.json")
BITS = {"bls12_381": 255, "bn254": 254}
# (own_records, g1_loose, pairs_built, pairs_default, words, bucket_bytes, coord_bytes): G1 in 14 limbs of 28 bits / 9 of 29;
# G2 over limbs of 28 bits: 2 x 14 / 2 x 10
FIELDS = {("bls12_381", False): FIELD_G1, ("bn254", False): (1, 1, 0, 0, 9, 4 * 9 * 4, 32),
          ("bls12_381", True): (1, 0, 1, 1, 28, 4 * 28 * 4, 96), ("bn254", True): (1, 0, 1, 0, 20, 4 * 20 * 4, 64)}
RESIDENT_GROUPS = {"bls12_381": 2, "bn254": 2, "bls12_381_g2": 1, "bn254_g2": 2}
# the sort's kernels (msm_driver.hpp sort_group: they follow from the plan alone and are not routed)
SORT = ("k_breakdown", "k_histA", "k_scan_slabs", "k_scan_parts", "k_scatterA", "k_scatterA_staged", "k_sortB", "k_big_find",
        "k_big_hist", "k_big_scan", "k_big_scatter")
PLAN_KEYS = {"window_bits": "wbits", "windows": "nwins", "buckets_per_window": "NB", "run_length": "L", "partitions": "NA",
             "low_bits": "LB", "fan_in": "F", "bucket_chunk": "K", "slabs": "nslabs", "slab_points": "slab_sz", "record_index_bits": "IB",
             "lg_slabs_per_group": "SH", "index_groups": "NG", "window_groups": "G", "first_bucket_chunk": "K1"}


def _kernel_id(name):
    """trace name `k_accumulate<montx_dev<...>, true>` -> MK_ACCUMULATE_FLAGGED; None: not one of this library's kernels"""
    m = re.match(r"(k_\w+)(<.*>)?$", name)
    if not m:
        return None
    base, targs = m.group(1), m.group(2) or ""
    if base in ("k_convert_points", "k_convert_points_staged", "k_accumulate"):
        return "MK_" + base[2:].upper().replace("_POINTS", "") + ("_FLAGGED" if targs.endswith(", true>") else "")
    return "MK_" + base[2:].upper()


def test_tail_code_decoder(plan_lib):
    names = ("no_join", "no_narrow_end", "no_latency_sums", "no_coop", "no_piece_tree", "convert_per_lane", "top_per_sum",
             "piece_level_launches", "sums_one_lane")
    table = {1: {"no_join", "no_piece_tree"}, 2: {"no_narrow_end"}, 3: {"no_latency_sums"}, 4: {"no_coop"}, 5: {"no_piece_tree"},
             6: {"convert_per_lane"}, 7: {"top_per_sum"}, 8: {"piece_level_launches"}, 10: {"sums_one_lane"}}
    out = (ctypes.c_uint * 11)()
    for code in range(0, 81):
        ok = plan_lib.emu_decode_tail_code(code, out)
        assert ok == (code < 80), code
        if not ok:
            continue
        assert {n for n, v in zip(names, out) if v} == table.get(code, set()), code         # (9, 11 ... 15: no switch)
        assert out[9] | out[10] << 32 == (1 << (code - 16) if code >= 16 else 32768), code  # PIECE_FUSE_MAX
    for code in (80, 81, 1000, 0xffffffff):
        assert not plan_lib.emu_decode_tail_code(code, out)
        assert plan_tuned(plan_lib, 4096, 255, code=code) is None


@pytest.fixture(scope="module")
def trace():
    return json.load(open(TRACE))


def test_route_predicts_the_recorded_launches(plan_lib, trace):
    cols = trace["columns"]
    ix = {c: cols.index(c) for c in ("name", "grid_size_x", "grid_size_y", "workgroup_size_x", "group_segment_size")}
    # lanes of k_accumulate the device holds at once, as the driver computes them: (work-groups of 256 lanes per CU its
    # occupancy query answered, at most 2) x 256 x CUs.  Pinned by the recorded plans (G1) and accumulation grids (alt_bn128
    # G2; BLS12-381 G2 takes its run lengths from the wave-pair kernel's own table at the recorded sizes: either value passes).
    resident = {k: v * 256 * trace["device"]["compute_units"] for k, v in RESIDENT_GROUPS.items()}
    ids = [_kernel_id(n) for n in trace["names"]]
    assert len(trace["cases"]) >= 170
    nlds = 0
    for c in trace["cases"]:
        curve, n, g2 = c["curve"], c["n"], bool(c["g2"])
        field, bits = FIELDS[(curve, g2)], BITS[curve]
        tun = dict(groups=c["groups"], K1=c["k1"], top=c["top"], code=c["code"], g2_path=c["g2"], long_runs=int(g2 and field[3]))
        # 1, 2: the plan from the recorded inputs is the plan the device's context reported
        p = plan_tuned(plan_lib, n, bits, resident["%s%s" % (curve, "_g2" if g2 else "")], **tun)
        if c["plan"] is not None:
            assert {k: p[v] for k, v in PLAN_KEYS.items()} == {k: c["plan"][k] for k in PLAN_KEYS}, c
        call = dict(may_defer=1, convert=1, flagged=int(c["stride"] > 2 * field[6]), stride=c["stride"], aligned16=int(c["offset"] % 16 == 0))
        if c["fixed_wbits"]:                    # the one-window plan over the tables; the points are the context's own records
            W = c["fixed_windows"]
            out = (ctypes.c_uint * 21)()
            plan_lib.emu_make_fixed_plan(n, -(-bits // W), W, 18 * 1024, out)        # (register_stage only sets plan.big: the sort's)
            p = dict(zip(KEYS, out))
            call = dict(may_defer=0, fb_n=n, convert=0, stride=0)
        # 3: the route is the recorded dispatches
        head, steps = route(plan_lib, p, field, bits, **call, **tun)
        check_route(p, field, head, steps, c)
        if c["plan"] is not None and not c["fixed_wbits"]:
            assert head["piece_cmax"] == c["plan"]["piece_tree_max"], c
        want = steps[:head["front"] - 1]
        for g in range(p["G"]):                 # the accumulation: a launch per window group, the last group shorter
            want.append(dict(steps[head["front"] - 1], gy=min(p["wpg"], p["nwins"] - g * p["wpg"])))
        want += steps[head["front"]:]
        assert bool(c["redone"]) <= bool(head["pieces"]), c
        if c["redone"]:
            head2, steps2 = route(plan_lib, p, field, bits, **dict(call, redo=1, may_defer=0), **tun)
            check_route(p, field, head2, steps2, c)
            want += steps2
        rows = [d for d in c["dispatches"] if ids[d[ix["name"]]] and not trace["names"][d[ix["name"]]].split("<")[0] in SORT]
        got = [(ids[d[ix["name"]]], d[ix["grid_size_x"]], d[ix["grid_size_y"]], d[ix["workgroup_size_x"]]) for d in rows]
        assert got == [(s["kernel"], s["gx"] * s["block"], s["gy"], s["block"]) for s in want], c
        # dynamic LDS: the kernels that take any have no static LDS, so the recorded segment is the route's figure
        for s, d in zip(want, rows):
            assert s["lds"] == 0 or s["lds"] == d[ix["group_segment_size"]], (c, s, d)
        nlds += sum(1 for s in want if s["lds"])
    assert nlds > 100
