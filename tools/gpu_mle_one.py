"""Multilinear tables and sumcheck rounds (sppark_amd.mle) on device-resident tables, each operation next to a yardstick that
exists without it -- parent code or a device copy -- alternating in the same run:

  fold (LOW, HIGH)      a Tensor.copy_ of 0.75 n elements: the same bytes (n read, n / 2 written)
  evaluate, eq          poly.vec_scale over one table of n elements (they move half its bytes)
  round, PRODUCT d = 2  poly.vec_mul over the same two tables (two thirds of its bytes)
  round, EQ_MUL_SUB     poly.vec_mul_sub with k over operands of the same size (four fifths of its bytes)

Device buffers, a non-default stream, WARM calls first, then the median of ROUNDS rounds of CALLS calls between two events;
the spread is the fastest and the slowest round.  evaluate, eq and round return when the result is in place, so their
figures include that wait.
    python tools/gpu_mle_one.py FIELD ops LG [LG ...]
    python tools/gpu_mle_one.py FIELD sumcheck LG      a whole sumcheck: LG alternating round + fold calls, against the sum of
                                                       the single-call medians of the same sizes"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sppark_amd import mle, poly

field, what = sys.argv[1], sys.argv[2]
lgs = [int(v) for v in sys.argv[3:]]
ROUNDS, WARM = 7, 3
EB = poly._ELEM_BYTES[field]
torch.cuda.set_stream(torch.cuda.Stream())
S = torch.cuda.current_stream().cuda_stream


def column(n, seed):
    """n canonical elements of |field| on the device"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    if EB == 8:
        return torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    if EB == 4:
        return torch.randint(0, 0x78000001, (n,), dtype=torch.int32, device="cuda", generator=g)
    if EB == 16:
        return torch.randint(0, 0x78000001, (n * 4,), dtype=torch.int32, device="cuda", generator=g)
    x = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)          # below 2^252 < every modulus
    x[:, 3] &= (1 << 59) - 1
    return x.reshape(n * 4)


def timed(fns, calls):
    """{name: (median, fastest, slowest)} ms per call; the operations alternate inside a round"""
    for _, fn in fns:
        for _ in range(WARM): fn()
    ms = {name: [] for name, _ in fns}
    for _ in range(ROUNDS):
        for name, fn in fns:
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls): fn()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / calls)
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}


def cell(t):
    return "%.4f [%.4f .. %.4f]" % t


def copier(elements):
    src = torch.empty(elements * EB, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.zero_()
    return lambda: dst.copy_(src, non_blocking=True)


def gate(ratio, bound, gated):
    return "%.3f (%s)" % (ratio, ("met" if ratio <= bound else "MISSED") + ", gate %.2f" % bound if gated else "no gate")


W = EB // column(1, 0).element_size() if EB >= 16 else 1
print("# %s %s; device %s; %d rounds, median [fastest .. slowest] ms per call"
      % (field, what, torch.cuda.get_device_name(0), ROUNDS), flush=True)
gated = EB <= 8
if what == "ops":
    for lg in lgs:
        n = 1 << lg
        calls = 20 if lg <= 22 else 8
        e, a, b, c = (column(n, lg + i) for i in range(4))
        out = torch.empty_like(a)
        half = torch.empty_like(a[:a.shape[0] // 2])
        point = column(lg, 77)
        k = column(1, 9).cpu().numpy()
        fns = [("fold_low", lambda: mle.fold(half, a, k, order=mle.LOW, field=field, stream=S)),
               ("copy0.75", copier(n // 2 + n // 4)),
               ("fold_high", lambda: mle.fold(half, a, k, order=mle.HIGH, field=field, stream=S)),
               ("evaluate", lambda: mle.evaluate(a, point, field=field, stream=S)),
               ("scale", lambda: poly.vec_scale(out, a, k, field=field, stream=S)),
               ("eq", lambda: mle.eq(out, point, field=field, stream=S)),
               ("round2", lambda: mle.round([a, b], field=field, stream=S)),
               ("mul", lambda: poly.vec_mul(out, a, b, field=field, stream=S)),
               ("round_ems", lambda: mle.round([e, a, b, c], form="eq_mul_sub", field=field, stream=S)),
               ("mul_sub_k", lambda: poly.vec_mul_sub(out, a, b, c, k=k, field=field, stream=S))]
        t = timed(fns, calls)
        gbs = lambda name, arrays: arrays * n * EB / t[name][0] / 1e6
        r = lambda x, y: t[x][0] / t[y][0]
        print("  2^%-3d fold LOW %s  HIGH %s  copy of 0.75 n %s  LOW/copy %s  HIGH/copy %s  (fold %.0f GB/s, copy %.0f GB/s)"
              % (lg, cell(t["fold_low"]), cell(t["fold_high"]), cell(t["copy0.75"]), gate(r("fold_low", "copy0.75"), 1.15, gated),
                 gate(r("fold_high", "copy0.75"), 1.15, gated), gbs("fold_high", 1.5), gbs("copy0.75", 1.5)), flush=True)
        print("        evaluate %s  eq %s  vec_scale %s  evaluate/scale %s  eq/scale %s  (evaluate %.0f GB/s, eq %.0f GB/s)"
              % (cell(t["evaluate"]), cell(t["eq"]), cell(t["scale"]), gate(r("evaluate", "scale"), 1.0, gated), gate(r("eq", "scale"), 1.0, gated),
                 gbs("evaluate", 1), gbs("eq", 1)), flush=True)
        print("        round PRODUCT d=2 %s  vec_mul %s  ratio %s  (%.0f GB/s);  round EQ_MUL_SUB %s  vec_mul_sub(k) %s  ratio %s  (%.0f GB/s)"
              % (cell(t["round2"]), cell(t["mul"]), gate(r("round2", "mul"), 1.0, gated), gbs("round2", 2), cell(t["round_ems"]),
                 cell(t["mul_sub_k"]), gate(r("round_ems", "mul_sub_k"), 1.0, gated), gbs("round_ems", 4)), flush=True)
else:
    lg = lgs[0]
    n = 1 << lg
    a, b = column(n, 1), column(n, 2)
    k = column(1, 9).cpu().numpy()
    wa, wb = a.clone(), b.clone()

    def whole():
        wa.copy_(a); wb.copy_(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        size = n * W
        for _ in range(lg):
            va, vb = wa[:size], wb[:size]
            mle.round([va, vb], order=mle.HIGH, field=field, stream=S)
            mle.fold(va, va, k, order=mle.HIGH, field=field, stream=S)
            mle.fold(vb, vb, k, order=mle.HIGH, field=field, stream=S)
            size //= 2
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(WARM): whole()
    runs = sorted(whole() for _ in range(ROUNDS))
    total = 0.0
    for j in range(lg, 0, -1):
        va, vb = wa[:(1 << j) * W], wb[:(1 << j) * W]
        t = timed([("round", lambda: mle.round([va, vb], order=mle.HIGH, field=field, stream=S)),
                   ("fold", lambda: mle.fold(va, va, k, order=mle.HIGH, field=field, stream=S))], 8)
        total += t["round"][0] + 2 * t["fold"][0]
    print("  2^%-3d whole sumcheck of two tables (%d x round + 2 folds) %.4f [%.4f .. %.4f] ms; sum of the single-call medians %.4f ms; "
          "gap %.4f ms" % (lg, lg, runs[len(runs) // 2], runs[0], runs[-1], total, runs[len(runs) // 2] - total), flush=True)
