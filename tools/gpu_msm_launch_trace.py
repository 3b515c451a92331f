"""The kernel launches of an MSM at both sides of every routing threshold, as data: what tests/golden/msm_launch_trace.json
records and tests/test_msm_route.py holds the route (csrc/msm/msm_route.hpp) against.

    rocprofv3 --kernel-trace -d OUT -- python tools/gpu_msm_launch_trace.py run [cases.json]
    python tools/gpu_msm_launch_trace.py extract OUT/.../*.db trace.json [cases.json]

`run` executes CASES -- single-chunk MSMs on seeded device-resident inputs -- in one process and writes what it ran (inputs,
the plan ctx.plan(n) reported, second passes) to cases.json (default build/msm_launch_trace_cases.json).  Every input
and the fixed-base tables are prepared BEFORE the first MSM, so from the first k_breakdown on the device runs nothing
but MSMs.  `extract` reads the dispatch table of the profiler's database as tools/rocprof_timeline.py does, in issue order, and cuts it at
the k_breakdown dispatches: every invoke opens with one per window group (one, but for the case with two groups), and
cases.json says how many a case has.  Two runs of the same cases on the same device -- two commits -- must give the same
trace.json.  Dispatches are (index into "names", grid x, grid y, work-group size[, LDS bytes]); grids in work-items, as
the profiler reports them."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1 << 10, 1 << 12, 5000, 1 << 13, 1 << 14, (1 << 15) + 17, 1 << 16, 1 << 17, 1 << 18, 300000, 1 << 19, 1 << 20,
         1 << 22, 1 << 23)
SMALL = tuple(n for n in SIZES if n <= 1 << 18)
# tune_tail codes (csrc/msm/msm_plan.hpp decode_tail_code): 1 no join, 2 no narrow end, 3 no low-latency sums, 4 no cooperative
# kernels, 5 no piece tree, 6 per-lane conversion, 7 top per sum, 8 a launch per piece level, 10 sums on one lane,
# 16 + x fuse the piece tail from 2^x work items
OTHER_CODES = (1, 2, 3, 5, 6, 7, 8, 10, 26, 46)


def cases():
    out = []

    def case(curve, n, code=0, g2=0, scalars="uniform", top=0, k1=0, groups=0, flagged=False, offset=0, fixed_wbits=0):
        out.append(dict(curve=curve, g2=g2, n=n, scalars=scalars, code=code, top=top, k1=k1, groups=groups, flagged=flagged,
                        offset=offset, fixed_wbits=fixed_wbits))
    for curve in ("bls12_381", "bn254"):
        for n in SIZES:
            for code in (0, 4):
                case(curve, n, code)
    for code in OTHER_CODES:
        for n in SMALL:
            case("bls12_381", n, code)
    for n in (1 << 12, 1 << 16):
        for code in (0, 8):
            case("bls12_381", n, code, scalars="equal")
    case("bls12_381", 1 << 18, top=1)
    case("bls12_381", 40000, k1=4)
    case("bls12_381", 40000, k1=16)
    case("bls12_381", 1 << 18, groups=2)
    case("bls12_381", 1 << 16, flagged=True)
    case("bls12_381", 1 << 12, offset=8)
    case("bls12_381", 5000, fixed_wbits=13)
    for curve in ("bls12_381", "bn254"):
        for path in (1, 2):
            for n in (1 << 12, 1 << 16, 1 << 18, 1 << 20):
                case(curve, n, g2=path)
    return out


def run(meta_path):
    import torch
    import sppark_amd
    from sppark_amd import synth
    cs = cases()
    stream = torch.cuda.current_stream().cuda_stream
    inputs, ctxs, fixed = {}, {}, {}
    for curve in ("bls12_381", "bn254"):
        fb = synth.FP_BYTES[curve]
        top = max(c["n"] for c in cs if c["curve"] == curve)
        pts, _ = synth.replicated_points(top, curve)
        sc = synth.uniform_scalars(top, curve, seed=77)
        d = dict(pts=pts, sc=sc, equal={}, flagged={}, offset={}, g2={})
        for c in cs:
            n = c["n"]
            if c["curve"] != curve:
                continue
            if c["scalars"] == "equal" and n not in d["equal"]:
                eq = sc[:n].clone(); eq[:] = sc[1]
                d["equal"][n] = eq
            if c["flagged"] and n not in d["flagged"]:
                fl = torch.zeros((n, 2 * fb + 8), dtype=torch.uint8, device="cuda")
                fl[:, :2 * fb] = pts[:n]
                fl[3, 2 * fb] = 1
                d["flagged"][n] = fl
            if c["offset"] and n not in d["offset"]:
                raw = torch.zeros(c["offset"] + n * 2 * fb, dtype=torch.uint8, device="cuda")
                raw[c["offset"]:] = pts[:n].reshape(-1)
                d["offset"][n] = raw[c["offset"]:]
                assert d["offset"][n].data_ptr() % 16 == c["offset"]
            if c["g2"] and n not in d["g2"]:
                # coordinates below 2^(8 fb - 8): the launches do not depend on the points being on the curve
                g = torch.Generator(device="cuda"); g.manual_seed(5)
                p2 = torch.randint(0, 256, (n, 4 * fb + 8), dtype=torch.uint8, device="cuda", generator=g)
                for k in range(1, 5):
                    p2[:, k * fb - 1] = 0
                p2[:, 4 * fb:] = 0
                d["g2"][n] = p2
        inputs[curve] = d
        ctxs[curve] = sppark_amd.MsmContext(curve, stream=stream)
        for c in cs:
            if c["curve"] == curve and c["fixed_wbits"]:
                f = sppark_amd.MsmContext(curve, stream=stream)
                f.tune(wbits=c["fixed_wbits"])
                f.set_points(pts[:c["n"]], fixed_base=True)
                f.tune(wbits=0)
                fixed[(curve, c["n"], c["fixed_wbits"])] = f
    torch.cuda.synchronize()
    props = torch.cuda.get_device_properties(0)
    meta = dict(device=dict(name=props.name, compute_units=props.multi_processor_count), cases=[])
    for c in cs:
        curve, n = c["curve"], c["n"]
        d = inputs[curve]
        rec = dict(c)
        if c["g2"]:
            sppark_amd.set_g2_path(c["g2"], curve)
            sppark_amd.multi_scalar_mult_fp2_arkworks(d["g2"][n], d["sc"][:n], curve)
            sppark_amd.set_g2_path(0, curve)
            rec.update(plan=None, markers=1, redone=0, stride=4 * synth.FP_BYTES[curve] + 8)
        else:
            ctx = fixed[(curve, n, c["fixed_wbits"])] if c["fixed_wbits"] else ctxs[curve]
            ctx.tune(); ctx.tune_sums(c["top"]); ctx.tune_tail(c["code"], c["k1"]); ctx.tune_pipeline(groups=c["groups"])
            sc = d["equal"][n] if c["scalars"] == "equal" else d["sc"][:n]
            pts = None if c["fixed_wbits"] else d["flagged"][n] if c["flagged"] else d["offset"][n] if c["offset"] else d["pts"][:n]
            stride = 2 * synth.FP_BYTES[curve] + (8 if c["flagged"] else 0)
            plan = ctx.plan(n)
            before = ctx.tail_redone()
            ctx.invoke(pts, sc, npoints=n, ffi_affine_sz=stride)
            redone = ctx.tail_redone() - before
            assert ctx.last_chunks() == 1, c
            if c["scalars"] == "equal":
                assert redone == 1, (c, redone)
            rec.update(plan=plan, markers=1 if c["fixed_wbits"] else plan["window_groups"], redone=redone, stride=stride,
                       fixed_windows=ctx.fixed_base_windows())
        torch.cuda.synchronize()
        meta["cases"].append(rec)
    for ctx in list(ctxs.values()) + list(fixed.values()):
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(meta_path)), exist_ok=True)
    with open(meta_path, "w") as f:
        json.dump(meta, f)
    print("ran %d cases -> %s" % (len(cs), meta_path))


def _kernel(name):
    """the kernel with its template arguments, without `void`, the namespace and the parameter list"""
    name = re.sub(r"(\s*\[clone \.kd\]|\.kd)$", "", name.strip())
    if name.startswith("_Z"):
        import subprocess
        name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += name[i] == ")"
            depth -= name[i] == "("
            if depth == 0:
                name = name[:i]
                break
    return re.sub(r"^void ", "", name).replace("sppark_amd::", "")


def dispatch_rows(db_path):
    """(columns, rows) of the profiler's dispatch table in issue order: a row is (kernel as _kernel() names it, grid x, grid y,
    work-group size[, LDS bytes]); also what tools/gpu_ntt_launch_trace.py cuts into cases"""
    import sqlite3
    db = sqlite3.connect(db_path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type in ('table','view')")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    have = [r[1] for r in db.execute("pragma table_info(%s)" % kd)]
    lds = [c for c in ("lds_block_size", "group_segment_size", "lds_size") if c in have]
    cols = ["grid_size_x", "grid_size_y", "workgroup_size_x"] + lds[:1]
    sym = [r[1] for r in db.execute("pragma table_info(%s)" % ks)]
    name_col = [c for c in ("demangled_kernel_name", "formatted_kernel_name", "display_name", "kernel_name") if c in sym][0]
    # in the order the host issued them: with two window groups the sort of the second runs on a stream of its own, and the
    # order of the START times of two streams differs from run to run
    rows = db.execute("select s.%s, %s from %s d join %s s on d.kernel_id = s.id order by d.%s"
                      % (name_col, ", ".join("d." + c for c in cols), kd, ks, "dispatch_id" if "dispatch_id" in have else "start")).fetchall()
    short = {n: _kernel(n) for n in {r[0] for r in rows}}
    return cols, [(short[r[0]],) + tuple(int(v) for v in r[1:]) for r in rows]


def extract(db_path, out_path, meta_path):
    meta = json.load(open(meta_path))
    cols, rows = dispatch_rows(db_path)
    marks = [i for i, r in enumerate(rows) if r[0].startswith("k_breakdown")]
    want = sum(c["markers"] for c in meta["cases"])
    assert len(marks) == want, (len(marks), want, sorted({r[0] for r in rows})[:40])
    names, out, m = [], [], 0
    for c in meta["cases"]:
        lo = marks[m]; m += c["markers"]
        hi = marks[m] if m < len(marks) else len(rows)
        disp = []
        for r in rows[lo:hi]:
            if r[0] not in names:
                names.append(r[0])
            disp.append([names.index(r[0])] + list(r[1:]))
        rec = {k: v for k, v in c.items() if k != "markers"}
        rec["dispatches"] = disp
        out.append(rec)
    with open(out_path, "w") as f:
        json.dump(dict(device=meta["device"], columns=["name"] + cols, names=names, cases=out), f, separators=(",", ":"))
    print("%d cases, %d dispatches, %d kernels -> %s" % (len(out), sum(len(c["dispatches"]) for c in out), len(names), out_path))


if __name__ == "__main__":
    default_meta = os.path.join(ROOT, "build", "msm_launch_trace_cases.json")
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(sys.argv[2] if len(sys.argv) > 2 else default_meta)
    elif len(sys.argv) >= 4 and sys.argv[1] == "extract":
        extract(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else default_meta)
    else:
        sys.exit(__doc__)
