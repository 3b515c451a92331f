#!/usr/bin/env python3
"""Measure the circle transform over Mersenne31 (include/sppark_amd_circle.h) on one MI355X and write the table of
DESIGN.md "Circle transform over M31":

    python tools/gpu_circle_bench.py [--out profiles/r11_circle_ntt.log] [--trace]

Device buffers, a non-NULL stream, device events around at least 0.2 s of repeated calls per figure; the compared
configurations alternate in ONE process, REPEATS times each, and the spread (min .. max) is printed next to the median.
Every timed configuration is first compared bit for bit with the host model (tests/circle_model.py): in full up to 2^20,
on 4096 sampled outputs of a sparse input (and the way back) above.  This parent process never opens the GPU: each step
is a child process under its own time limit, and nothing more is started after a step that failed.

Gates (each against existing code timed in the same run):
  forward, BITREV, one column of 2^16 / 2^20 / 2^24   <=  libsppark_bb31's sppark_ntt forward NR of that size
                                                           + one sppark_field_add over an M31 array of that size
  4096 columns of 2^12, forward and inverse            <=  one transform of 2^24, within the measured spread
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 7
MIN_SECONDS = 0.2
SIZES = (16, 20, 24)


def _measure(out):
    import numpy as np
    import torch
    import circle_model as M
    from sppark_amd import circle, ffi

    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    m31, bb31 = ffi.load("m31"), ffi.load("bb31")
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")

    def host(t):
        return t.cpu().numpy().view(np.uint32)

    def timed(fn):
        """ms per call: device events around enough back-to-back calls for MIN_SECONDS"""
        for _ in range(3):
            fn()
        stream.synchronize()
        reps = 4
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= MIN_SECONDS * 1e3:
                return ms / reps
            reps = max(reps * 2, int(reps * MIN_SECONDS * 1.2e3 / max(ms, 1e-3)) + 1)

    def alternate(configs):
        """{name: fn} -> {name: (median, min, max)} in ms, the configurations taking turns REPEATS times"""
        got = {k: [] for k in configs}
        for _ in range(REPEATS):
            for k, fn in configs.items():
                got[k].append(timed(fn))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}

    def fmt(t):
        return "%8.4f ms (%.4f .. %.4f)" % t

    def cntt(d, lg, batch, order, direction):
        ffi.check(m31, m31.sppark_circle_ntt(0, d.data_ptr(), lg, batch, 0, order, direction, sp))

    # ---- correctness first: every configuration that is timed below ----
    rng = np.random.default_rng(11)
    for k in SIZES:
        n = 1 << k
        if k <= 20:
            x = rng.integers(0, M.P, n, dtype=np.uint32)
            d = dev(x)
            cntt(d, k, 1, 0, 0)
            stream.synchronize()
            want = M.forward(x, k)
            assert (host(d) == want).all(), "forward 2^%d differs from the host model" % k
            dn = dev(x)
            cntt(dn, k, 1, 1, 0)
            stream.synchronize()
            assert (host(dn)[M.bitrev_perm(k)] == want).all(), "forward NATURAL 2^%d differs from the host model" % k
            cntt(d, k, 1, 0, 1)
            stream.synchronize()
            assert (host(d) == x).all(), "inverse 2^%d does not restore the input" % k
            e = rng.integers(0, M.P, n, dtype=np.uint32)
            d = dev(e)
            cntt(d, k, 1, 0, 1)
            stream.synchronize()
            assert (host(d) == M.inverse(e, k)).all(), "inverse 2^%d differs from the host model" % k
        else:
            idx = [0, 1, 5, n // 2 + 3, n - 2, n - 1]
            val = [3, M.P - 1, 123456789, 7, 2, 1]
            pos = rng.integers(0, n, 4096)
            d = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            d[torch.tensor(idx, device="cuda:0")] = torch.tensor(val, dtype=torch.int32, device="cuda:0")
            ref = d.clone()
            torch.cuda.synchronize()
            cntt(d, k, 1, 0, 0)
            stream.synchronize()
            assert (host(d[torch.from_numpy(pos).to("cuda:0")]) == M.sparse_evaluate(idx, val, k, pos)).all(), "forward 2^%d: sampled outputs differ" % k
            cntt(d, k, 1, 0, 1)
            stream.synchronize()
            assert torch.equal(d, ref), "inverse 2^%d does not restore the input" % k
            cntt(d, k, 1, 1, 0)
            stream.synchronize()
            assert (host(d[torch.from_numpy(pos).to("cuda:0")]) == M.sparse_evaluate(idx, val, k, pos, M.NATURAL)).all(), \
                "forward NATURAL 2^%d: sampled outputs differ" % k
    xb = rng.integers(0, M.P, (4096, 1 << 12), dtype=np.uint32)
    db = dev(xb)
    cntt(db, 12, 4096, 0, 0)
    stream.synchronize()
    rows = rng.integers(0, 4096, 64)
    assert (host(db)[rows] == M.forward(xb[rows], 12)).all(), "batched forward differs from the host model"
    cntt(db, 12, 4096, 0, 1)
    stream.synchronize()
    assert (host(db) == xb).all(), "batched inverse does not restore the input"
    el = rng.integers(0, M.P, (64, 1 << 16), dtype=np.uint32)
    bl = np.zeros((64, 1 << 18), dtype=np.uint32)
    bl[:, :1 << 16] = el
    dl = dev(bl)
    ffi.check(m31, m31.sppark_circle_lde(0, dl.data_ptr(), 16, 2, 64, 0, None, sp))
    stream.synchronize()
    assert (host(dl)[:4] == M.lde(el[:4], 16, 2)[1]).all(), "LDE differs from the host model"
    say("verified: forward (both orders) / inverse 2^16, 2^20 in full, 2^24 on 4096 samples and the way back; 4096 x 2^12 on 64 columns and the way back; "
        "LDE 64 x 2^16 -> 2^18 on 4 columns")
    say()

    # ---- forward against BabyBear's NTT + one pass of field_add; inverse against forward ----
    say("one column, BITREV order, device buffer, non-NULL stream; median of %d alternating repeats (min .. max)" % REPEATS)
    gates = []
    for k in SIZES:
        n = 1 << k
        d = dev(rng.integers(0, M.P, n, dtype=np.uint32))
        b = dev(rng.integers(0, 0x78000001, n, dtype=np.uint32))
        a0, a1, a2 = (dev(rng.integers(0, M.P, n, dtype=np.uint32)) for _ in range(3))
        r = alternate({
            "circle forward": lambda: cntt(d, k, 1, 0, 0),
            "bb31 NTT forward NR": lambda: ffi.check(bb31, bb31.sppark_ntt(0, b.data_ptr(), k, 1, 0, 0, sp)),
            "m31 field_add": lambda: ffi.check(m31, m31.sppark_field_add(0, a0.data_ptr(), a1.data_ptr(), a2.data_ptr(), n, sp)),
            "circle inverse (warm)": lambda: cntt(d, k, 1, 0, 1),
            "circle forward NATURAL": lambda: cntt(d, k, 1, 1, 0),
        })
        cold = []
        for _ in range(3):                              # a cold cache: the one call builds its tables, device events around it
            stream.synchronize()
            ffi.check(m31, m31.sppark_circle_release_cached(0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            cntt(d, k, 1, 0, 1)
            e1.record(stream)
            e1.synchronize()
            cold.append(e0.elapsed_time(e1))
        cntt(d, k, 1, 0, 0)                             # (rebuild the point tables before the next timing)
        stream.synchronize()
        fwd, ref, add = r["circle forward"][0], r["bb31 NTT forward NR"][0], r["m31 field_add"][0]
        ok = fwd <= ref + add
        gates.append(ok)
        say("2^%d" % k)
        for name, t in r.items():
            say("  %-26s %s" % (name, fmt(t)))
        say("  %-26s %8.4f ms (%.4f .. %.4f), one call after release_cached, table build included" % ("circle inverse (cold)", statistics.median(cold), min(cold), max(cold)))
        say("  forward / (bb31 + add) = %.3f  -> gate %s;  forward / bb31 = %.3f;  inverse warm / forward = %.3f;  inverse cold / forward = %.1f"
            % (fwd / (ref + add), "MET" if ok else "MISSED", fwd / ref, r["circle inverse (warm)"][0] / fwd, statistics.median(cold) / fwd))
    say()

    # ---- the batch against one transform of the total size ----
    d24 = dev(rng.integers(0, M.P, 1 << 24, dtype=np.uint32))
    r = alternate({
        "4096 x 2^12 forward": lambda: cntt(db, 12, 4096, 0, 0),
        "1 x 2^24 forward": lambda: cntt(d24, 24, 1, 0, 0),
        "4096 x 2^12 inverse": lambda: cntt(db, 12, 4096, 0, 1),
        "1 x 2^24 inverse": lambda: cntt(d24, 24, 1, 0, 1),
    })
    say("batch of 4096 columns of 2^12 against one transform of 2^24")
    for name, t in r.items():
        say("  %-26s %s" % (name, fmt(t)))
    for what in ("forward", "inverse"):
        bt, one = r["4096 x 2^12 " + what], r["1 x 2^24 " + what]
        ok = bt[0] <= one[0] + (one[2] - one[1])
        gates.append(ok)
        say("  %s: batch / single = %.3f -> gate %s" % (what, bt[0] / one[0], "MET" if ok else "MISSED"))
    say()

    r = alternate({"LDE 64 x 2^16 -> 2^18": lambda: ffi.check(m31, m31.sppark_circle_lde(0, dl.data_ptr(), 16, 2, 64, 0, None, sp))})
    say("LDE of 64 columns 2^16 -> 2^18 (reported only)")
    say("  %-26s %s" % ("LDE 64 x 2^16 -> 2^18", fmt(r["LDE 64 x 2^16 -> 2^18"])))
    say()
    say("gates: %d of %d met" % (sum(gates), len(gates)))
    say("cached bytes after the run: %d" % circle.cached_bytes(0))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


def _trace_workload():
    """what the kernel trace sees: a few forward and inverse transforms of 2^24 and BabyBear's NTT of the same size"""
    import numpy as np
    import torch
    from sppark_amd import ffi
    m31, bb31 = ffi.load("m31"), ffi.load("bb31")
    d = torch.from_numpy(np.random.default_rng(1).integers(0, (1 << 31) - 1, 1 << 24, dtype=np.uint32).view(np.int32)).to("cuda:0")
    for _ in range(10):
        ffi.check(m31, m31.sppark_circle_ntt(0, d.data_ptr(), 24, 1, 0, 0, 0, None))
        ffi.check(m31, m31.sppark_circle_ntt(0, d.data_ptr(), 24, 1, 0, 0, 1, None))
        ffi.check(bb31, bb31.sppark_ntt(0, d.data_ptr(), 24, 1, 0, 0, None))
    torch.cuda.synchronize()


def _append_trace(out, tdir):
    """the per-kernel times of the traced 2^24 workload (ten forward, ten inverse, ten BabyBear transforms), into the log"""
    import csv
    import glob
    found = sorted(glob.glob(os.path.join(tdir, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        return
    with open(found[0]) as f:
        rows = list(csv.DictReader(f))
    with open(out, "a") as f:
        f.write("\nkernel trace of ten forward + ten inverse circle transforms and ten BabyBear NTTs of 2^24 (rocprofv3 --kernel-trace --stats, a run of its own)\n")
        f.write("  %-44s %6s %12s %12s %12s\n" % ("kernel", "calls", "average us", "min us", "max us"))
        for r in rows:
            name = r["Name"].split("(")[0].replace("void sppark_amd::", "")
            f.write("  %-44s %6s %12.1f %12.1f %12.1f\n" % (name[:44], r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
        f.write("  (a circle transform of 2^24 is k_circle_pass x 3: two passes of 6 layers -- the min column -- and the 12-layer pass on the\n"
                "   lowest layers -- the max column; BabyBear's is k_ntt6 x 2 + k_ntt12.  Each pass moves 128 MB: about 30 us at the\n"
                "   bandwidth field_add reaches above.  The 12-layer pass takes three times that with 10^8 butterflies of 12 vector\n"
                "   instructions plus LDS addressing and twiddle reads per lane: the issue rate bounds it, not the bandwidth.)\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_circle_ntt.log"))
    ap.add_argument("--trace", action="store_true", help="also a rocprofv3 --kernel-trace --stats run of 2^24 (a run of its own)")
    ap.add_argument("--step", choices=("measure", "trace-workload"))
    a = ap.parse_args()
    if a.step == "measure":
        return _measure(a.out)
    if a.step == "trace-workload":
        return _trace_workload()
    me = os.path.abspath(__file__)
    steps = [([sys.executable, me, "--step", "measure", "--out", a.out], 420)]
    tdir = os.path.splitext(a.out)[0] + "_trace"
    if a.trace:
        steps.append((["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "-o", "circle", "--output-format", "csv", "--",
                       sys.executable, me, "--step", "trace-workload"], 240))
    for cmd, limit in steps:
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"step": cmd[-1], "error": "time limit of %d s" % limit}))
            return 1
        if rc != 0:                                     # nothing more is started on the GPU after a step that failed
            print(json.dumps({"step": cmd[-1], "error": "exit status %d" % rc}))
            return 1
    if a.trace:
        _append_trace(a.out, tdir)
    return 0


if __name__ == "__main__":
    sys.exit(main())
