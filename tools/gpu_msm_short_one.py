"""MSM over short scalars against the full-width call on the same values: the measurement of DESIGN.md "Short scalars".

    python tools/gpu_msm_short_one.py [--log profiles/r10_msm_short_scalars.log] [--parent-libdir lib_parent] [--only cells|sweep|headline]

The driver runs one GPU step at a time, each a child process of this file under its own `timeout`, appends what the step
prints to the log and stops at the first step that fails.  Steps:

    cells CURVE LG        2^LG points, b = 32, 64, 128 (alt_bn128: 64): inputs on the device, the context reserved beforehand,
                          7 rounds of [short call, yardstick] alternating; the yardstick is the ordinary invoke on the same
                          scalars zero-extended to 32 bytes.  Per call: wall ms (median, fastest, slowest), kernel_ms(0 / 1 / 2)
                          of the median round, windows; short / yardstick
    sweep                 tune(wbits=) -3 .. +3 around the automatic width at 2^20 points, b = 64 (recorded only)
    headline LIBDIR       the ordinary full-width 2^26 call, alternately from the libraries in sppark_amd/LIBDIR (a build of
                          the parent commit: SPPARK_LIBDIR, sppark_amd/build.py) and from this tree's, 7 rounds
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 7
NAMES = {"bls12_381": "BLS12-381", "bn254": "alt_bn128"}


def _inputs(name, n, fb):
    import torch
    import sppark_amd
    base = torch.zeros((2048, 2 * fb), dtype=torch.uint8, device="cuda")
    sppark_amd.generate_points(base, 2048, 0x5eed5eed0001, 2 * fb, name)
    pts = base[torch.arange(n, device="cuda") % 2048].contiguous()
    g = torch.Generator(device="cuda"); g.manual_seed(n & 0xffff)
    words = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    return pts, words


def _timed(ctx, call):
    t0 = time.perf_counter()
    call()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, [ctx.kernel_ms(k) for k in (0, 1, 2)]


def _summary(rows):
    """rows of (wall, [k0, k1, k2]) -> median wall, fastest, slowest, kernel times of the median round"""
    rows = sorted(rows, key=lambda r: r[0])
    mid = rows[len(rows) // 2]
    return mid[0], rows[0][0], rows[-1][0], mid[1]


def step_cells(name, lg):
    import torch
    import sppark_amd
    fb = sppark_amd.msm.FP_BYTES[name]
    n = 1 << lg
    pts, words = _inputs(name, n, fb)
    ctx = sppark_amd.MsmContext(name)
    ctx.enable_timing(True)
    ctx.reserve(n, 2 * fb)                              # the larger of the two plans
    for b in ((64,) if name == "bn254" else (32, 64, 128)):
        w = (b + 63) // 64
        short = words[:, :w].contiguous()               # n x 8 or 16 bytes; b = 32: the low word of an 8-byte slot ...
        if b == 32:
            short = short.view(torch.int32)[:, :1].contiguous()      # ... as a 4-byte slot
        S = short.shape[1] * short.element_size()
        wide = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        wide[:, :w] = words[:, :w]
        if b == 32:
            wide[:, 0] &= 0xffffffff
        ctx.reserve(n, 2 * fb, scalar_bits=b, scalar_stride=S)
        torch.cuda.synchronize()
        f_short = lambda: ctx.invoke(pts, short, npoints=n, scalar_bits=b, scalar_stride=S)      # noqa: E731
        f_wide = lambda: ctx.invoke(pts, wide, npoints=n)                                         # noqa: E731
        a, c = f_short(), f_wide()                      # warm-up, and the two agree
        assert (sppark_amd.to_affine(a, name) == sppark_amd.to_affine(c, name)).all(), (name, lg, b)
        rs, rw = [], []
        for _ in range(ROUNDS):
            rs.append(_timed(ctx, f_short))
            rw.append(_timed(ctx, f_wide))
        ms, lo_s, hi_s, ks = _summary(rs)
        mw, lo_w, hi_w, kw = _summary(rw)
        ps, pw = ctx.plan(n, scalar_bits=b), ctx.plan(n)
        print("%s 2^%d b=%d stride=%d" % (NAMES[name], lg, b, S))
        print("    short      wall %8.3f ms (fastest %8.3f, slowest %8.3f)  kernel_ms before-accumulate %7.3f accumulate %8.3f device %8.3f  windows %2d x %2d bits"
              % (ms, lo_s, hi_s, ks[0], ks[1], ks[2], ps["windows"], ps["window_bits"]))
        print("    yardstick  wall %8.3f ms (fastest %8.3f, slowest %8.3f)  kernel_ms before-accumulate %7.3f accumulate %8.3f device %8.3f  windows %2d x %2d bits"
              % (mw, lo_w, hi_w, kw[0], kw[1], kw[2], pw["windows"], pw["window_bits"]))
        print("    short / yardstick %.3f   (windows %d / %d = %.3f; yardstick spread %.3f ms, gain %.3f ms)"
              % (ms / mw, ps["windows"], pw["windows"], ps["windows"] / pw["windows"], hi_w - lo_w, mw - ms), flush=True)
        del wide, short
    ctx.close()


def step_sweep():
    import torch
    import sppark_amd
    name, lg, b = "bls12_381", 20, 64
    n = 1 << lg
    pts, words = _inputs(name, n, 48)
    short = words[:, :1].contiguous()
    ctx = sppark_amd.MsmContext(name)
    ctx.enable_timing(True)
    auto = ctx.plan(n, scalar_bits=b)
    print("tune(wbits=) sweep, %s 2^%d b=%d: automatic %d windows x %d bits (from the full-width table: recorded only)"
          % (NAMES[name], lg, b, auto["windows"], auto["window_bits"]))
    # the automatic REQUEST is what make_plan asks for before the even split: the width whose window count the plan has
    for wb in range(max(2, auto["window_bits"] - 3), min(24, auto["window_bits"] + 3) + 1):
        ctx.tune(wbits=wb)
        p = ctx.plan(n, scalar_bits=b)
        ctx.reserve(n, 96, scalar_bits=b, scalar_stride=8)
        f = lambda: ctx.invoke(pts, short, npoints=n, scalar_bits=b, scalar_stride=8)             # noqa: E731
        f()
        wall, lo, hi, k = _summary([_timed(ctx, f) for _ in range(ROUNDS)])
        print("    wbits=%2d -> %2d windows x %2d bits  wall %7.3f ms (fastest %7.3f, slowest %7.3f)  kernel_ms %6.3f / %6.3f / %6.3f"
              % (wb, p["windows"], p["window_bits"], wall, lo, hi, k[0], k[1], k[2]), flush=True)
    ctx.close()
    torch.cuda.synchronize()


def step_headline(libdir):
    """through ctypes alone: the parent's library has none of the short-scalar symbols sppark_amd.ffi declares on loading"""
    import ctypes
    import numpy as np
    import torch
    import sppark_amd
    from sppark_amd import ffi
    name, n = "bls12_381", 1 << 26
    pts, words = _inputs(name, n, 48)
    sc = words.view(torch.uint8).reshape(n, 32)
    sc[:, 31] &= 0x3f                                   # < 2^254 < r
    torch.cuda.synchronize()
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    libs, ctxs = {}, {}
    for tag, path in (("parent", os.path.join(ROOT, "sppark_amd", libdir, "libsppark_%s.so" % name)), ("this", ffi.lib_path(name))):
        L = ctypes.CDLL(path)
        L.sppark_msm_create.argtypes = [ctypes.POINTER(vp), ci, vp]; L.sppark_msm_create.restype = ffi._Error
        L.sppark_msm_reserve.argtypes = [vp, sz, sz, ci, ci]; L.sppark_msm_reserve.restype = ffi._Error
        L.sppark_msm_invoke.argtypes = [vp, vp, vp, sz, vp, ci, sz]; L.sppark_msm_invoke.restype = ffi._Error
        L.sppark_msm_destroy.argtypes = [vp]
        L.drop_error_message.argtypes = [vp]
        h = vp()
        ffi.check(L, L.sppark_msm_create(ctypes.byref(h), -1, None))
        ffi.check(L, L.sppark_msm_reserve(h, n, 96, 0, 0))
        libs[tag], ctxs[tag] = L, h

    def invoke(tag):
        out = np.zeros(144, dtype=np.uint8)
        ffi.check(libs[tag], libs[tag].sppark_msm_invoke(ctxs[tag], out.ctypes.data, pts.data_ptr(), n, sc.data_ptr(), 0, 96))
        return out
    assert (sppark_amd.to_affine(invoke("parent"), name) == sppark_amd.to_affine(invoke("this"), name)).all()     # (the same point: the Jacobian form depends on the sort's order)
    rows = {t: [] for t in ctxs}
    for _ in range(ROUNDS):
        for t in ("parent", "this"):
            t0 = time.perf_counter()
            invoke(t)
            rows[t].append((time.perf_counter() - t0) * 1e3)
    print("the ordinary full-width call, %s 2^26, uniform scalars, parent build and this one alternating" % NAMES[name])
    for t in ("parent", "this"):
        print("    %-6s wall %8.3f ms (fastest %8.3f, slowest %8.3f)" % (t, statistics.median(rows[t]), min(rows[t]), max(rows[t])))
    print("    this / parent %.4f" % (statistics.median(rows["this"]) / statistics.median(rows["parent"])), flush=True)
    for t in ctxs:
        libs[t].sppark_msm_destroy(ctxs[t])


def main():
    if "--step" in sys.argv:
        a = sys.argv[sys.argv.index("--step") + 1:]
        {"cells": lambda: step_cells(a[1], int(a[2])), "sweep": step_sweep, "headline": lambda: step_headline(a[1])}[a[0]]()
        return 0
    log = os.path.join(ROOT, "profiles", "r10_msm_short_scalars.log")
    if "--log" in sys.argv:
        log = sys.argv[sys.argv.index("--log") + 1]
    parent = sys.argv[sys.argv.index("--parent-libdir") + 1] if "--parent-libdir" in sys.argv else None
    steps = [(["cells", "bls12_381", str(lg)], 120 if lg < 26 else 240) for lg in (16, 20, 22, 24, 26)]
    steps += [(["cells", "bn254", "24"], 120), (["sweep"], 120)]
    if parent:
        steps.append((["headline", parent], 240))
    if "--only" in sys.argv:                            # one kind of step, appended to the log
        steps = [s for s in steps if s[0][0] == sys.argv[sys.argv.index("--only") + 1]]
    with open(log, "a" if "--only" in sys.argv else "w") as f:
        if "--only" not in sys.argv:
            f.write("# tools/gpu_msm_short_one.py: short-scalar MSM against the full-width call on the same values, device-resident inputs,\n"
                    "# reserved context, median of %d alternating rounds (see the tool's docstring)\n" % ROUNDS)
        for args, limit in steps:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + args,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            f.write(r.stdout); f.flush()
            sys.stdout.write(r.stdout); sys.stdout.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                f.write("# step %s failed with exit status %d: stopped\n" % (" ".join(args), r.returncode))
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
