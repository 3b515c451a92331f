"""Batched NTT / LDE timings (sppark_ntt_batch / sppark_lde_batch) on device-resident buffers, device events on a non-NULL
stream.  Writes profiles/r07_ntt_batch.log (or the path given by --out).

    python tools/gpu_ntt_batch_bench.py                 the table: per field and mode, batches of 2^24 elements (2^22 for the
                                                        256-bit fields) at lg 2 ... 20 against ONE transform of the total
                                                        size and against the loop of per-column sppark_ntt calls; the LDEs
    python tools/gpu_ntt_batch_bench.py --trace         a few batched calls for a rocprofv3 --kernel-trace run (launches per call)
    python tools/gpu_ntt_batch_bench.py --ab DIR1 DIR2  single transforms, alternating two builds (sppark_amd/DIR1, DIR2) in
                                                        child processes: gl64, bb31, bls12_381 at 2^12, 2^20, 2^24
    python tools/gpu_ntt_batch_bench.py --packed DIR    the packed kernel against one work-group per column (a tuning build in
                                                        sppark_amd/DIR, -DSPPARK_TUNING: SPPARK_NTT_PACKED_MAX = 6 / 0
                                                        alternating in child processes), gl64 and bb31 at lg 1 ... 7

The per-column loop is timed over at most LOOP_MAX columns and scaled to the batch (a loop of 2^22 calls at lg 2 would take
minutes); the log says so."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOOP_MAX = 4096
MODES = (("fwd NR", 1, 0, 0), ("inv RN", 2, 1, 0), ("coset fwd NR", 1, 0, 1))
FIELDS = (("gl64", 8, 24), ("bb31", 4, 24), ("bls12_381", 32, 22))          # (field, bytes per element, log2 total elements)
LGS = (2, 5, 8, 11, 12, 16, 20)


def _torch():
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing to measure"
    return torch


def _buf(torch, eb, n_elems):
    words = n_elems * eb // (4 if eb == 4 else 8)
    return torch.randint(0, 2**30, (words,), dtype=torch.int32 if eb == 4 else torch.int64, device="cuda")


def _time(torch, fn, reps):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def table(out):
    torch = _torch()
    from sppark_amd import ffi
    torch.cuda.set_stream(torch.cuda.Stream())
    h = torch.cuda.current_stream().cuda_stream
    for field, eb, lg_tot in FIELDS:
        L = ffi.load(field)
        x = _buf(torch, eb, 1 << lg_tot)
        p = x.data_ptr()
        for name, order, direction, typ in MODES:
            one = _time(torch, lambda: ffi.check(L, L.sppark_ntt(0, p, lg_tot, order, direction, typ, h)), 20)
            out("%s %s: one transform of 2^%d  %.4f ms" % (field, name, lg_tot, one))
            for lg in LGS:
                batch = 1 << (lg_tot - lg)
                bt = _time(torch, lambda: ffi.check(L, L.sppark_ntt_batch(0, p, lg, batch, 0, order, direction, typ, h)), 20)
                cols = min(batch, LOOP_MAX)
                stride = eb << lg

                def loop():
                    for j in range(cols):
                        ffi.check(L, L.sppark_ntt(0, p + j * stride, lg, order, direction, typ, h))
                lt = _time(torch, loop, 2) * batch / cols
                out("  %s %s lg %2d x %8d: batch %.4f ms (%.2fx one transform)  loop %s%.3f ms  -> %.0fx" % (
                    field, name, lg, batch, bt, bt / one, "~" if cols < batch else "", lt, lt / bt))
        del x
        torch.cuda.empty_cache()
    # LDE: 64 columns of 2^16 -> 2^18 (gl64, bb31), 16 (bls12_381), against one LDE of the same totals and the loop
    for field, eb, b in (("gl64", 8, 64), ("bb31", 4, 64), ("bls12_381", 32, 16)):
        L = ffi.load(field)
        lgd, lgb = 16, 2
        lg_one = lgd + (b.bit_length() - 1)
        x = _buf(torch, eb, b << (lgd + lgb))
        p = x.data_ptr()
        one = _time(torch, lambda: ffi.check(L, L.sppark_lde(0, p, lg_one, lgb, None, h)), 10)
        bt = _time(torch, lambda: ffi.check(L, L.sppark_lde_batch(0, p, lgd, lgb, b, None, h)), 10)
        ext_b = eb << (lgd + lgb)

        def loop():
            for j in range(b):
                ffi.check(L, L.sppark_lde(0, p + j * ext_b, lgd, lgb, None, h))
        lt = _time(torch, loop, 3)
        out("%s LDE %d x (2^%d -> 2^%d): batch %.4f ms   one 2^%d -> 2^%d LDE %.4f ms   loop %.3f ms" % (
            field, b, lgd, lgd + lgb, bt, lg_one, lg_one + lgb, one, lt))
        del x
        torch.cuda.empty_cache()


def trace(out):
    """batched calls below the grid limit: the launch count per call must not grow with the batch (kernel trace)"""
    torch = _torch()
    from sppark_amd import ffi
    torch.cuda.set_stream(torch.cuda.Stream())
    h = torch.cuda.current_stream().cuda_stream
    L = ffi.load("gl64")
    for lg in (4, 12, 16):
        x = _buf(torch, 8, min(4096 << lg, 1 << 26))
        for b in (1, 16, 256, 4096):
            if (b << lg) > (1 << 26):
                continue
            for name, order, direction, typ in MODES:
                ffi.check(L, L.sppark_ntt_batch(0, x.data_ptr(), lg, b, 0, order, direction, typ, h))
            torch.cuda.synchronize()
            out("trace: gl64 lg %d batch %d: 3 calls (fwd NR, inv RN, coset fwd NR)" % (lg, b))
        del x


def single(out):
    """sppark_ntt only: the build before the batched entry points has no sppark_ntt_batch for ffi.load to declare"""
    import ctypes
    torch = _torch()
    from sppark_amd import ffi
    torch.cuda.set_stream(torch.cuda.Stream())
    h = torch.cuda.current_stream().cuda_stream
    for field, eb, _ in FIELDS:
        L = ctypes.CDLL(ffi.lib_path(field))
        L.sppark_ntt.argtypes = [ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.sppark_ntt.restype = ffi._Error
        L.drop_error_message.argtypes = [ctypes.c_void_p]
        for lg in (12, 20, 24):
            x = _buf(torch, eb, 1 << lg)
            p = x.data_ptr()
            res = []
            for name, order, direction, typ in MODES:
                res.append("%s %.4f" % (name, _time(torch, lambda: ffi.check(L, L.sppark_ntt(0, p, lg, order, direction, typ, h)), 50 if lg < 24 else 20)))
            out("%s %s 2^%d: %s ms" % (os.environ.get("SPPARK_LIBDIR", "lib"), field, lg, " | ".join(res)))
            del x


def packed(out):
    torch = _torch()
    from sppark_amd import ffi
    torch.cuda.set_stream(torch.cuda.Stream())
    h = torch.cuda.current_stream().cuda_stream
    res = []
    for field, eb, lg_tot in FIELDS[:2]:
        L = ffi.load(field)
        x = _buf(torch, eb, 1 << lg_tot)
        p = x.data_ptr()
        for lg in range(1, 8):
            batch = 1 << (lg_tot - lg)
            t = [_time(torch, lambda: ffi.check(L, L.sppark_ntt_batch(0, p, lg, batch, 0, order, direction, typ, h)), 20)
                 for _, order, direction, typ in MODES[:2]]
            res.append("%s lg %d x %d: fwd NR %.4f  inv RN %.4f" % (field, lg, batch, t[0], t[1]))
        del x
    out("SPPARK_NTT_PACKED_MAX=%s: %s ms" % (os.environ.get("SPPARK_NTT_PACKED_MAX"), " | ".join(res)))


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r07_ntt_batch.log")
    if "--out" in args:
        path = args[args.index("--out") + 1]
    f = open(path, "a")

    def out(line):
        print(line, flush=True)
        f.write(line + "\n"); f.flush()
    if "--trace" in args:
        trace(out)
    elif "--packed-one" in args:
        packed(out)
    elif "--packed" in args:
        d = args[args.index("--packed") + 1]
        out("packed kernel (SPPARK_NTT_PACKED_MAX=6) against one work-group per column (=0), build %s, batches of 2^24 elements" % d)
        for rnd in range(2):
            for v in ("6", "0"):
                env = dict(os.environ, SPPARK_LIBDIR=d, SPPARK_NTT_PACKED_MAX=v)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--packed-one", "--out", path], env=env, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("packed run failed with %d" % r.returncode)
    elif "--single" in args:
        single(out)
    elif "--ab" in args:
        i = args.index("--ab")
        dirs = args[i + 1:i + 3]
        out("single transforms, alternating builds %s / %s (device events, non-NULL stream, ms per call)" % tuple(dirs))
        for rnd in range(2):
            for d in dirs:
                env = dict(os.environ, SPPARK_LIBDIR=d)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--single", "--out", path], env=env, timeout=600)
                if r.returncode != 0:
                    raise SystemExit("single-transform run failed with %d" % r.returncode)
    else:
        out("batched NTT: batches of 2^24 elements (2^22 for BLS12-381) against one transform of that size and the per-column "
            "loop (~: timed over %d columns, scaled); device events, non-NULL stream, ms per call" % LOOP_MAX)
        table(out)


if __name__ == "__main__":
    main()
