"""Field-vector arithmetic, polynomial product and vanishing quotient on device-resident arrays, each next to a yardstick
that exists without them, timed in the same run:

  pointwise   a device-to-device copy that moves the same bytes (a three-operand operation reads two arrays and writes
              one: a copy of 1.5 arrays); for the 256-bit product also prefix_op(MULTIPLY) on the same array
  product     two forward NR and one inverse RN public transforms of the padded size, plus a copy of the bytes that
              padding, the pointwise product and the copy-out move
  quotient    the same seven transforms through compute_ntt_batch / compute_ntt, plus the same-bytes copy for staging,
              mul_sub and the copy into h

Device buffers, a non-default stream, WARM calls first, then the median of ROUNDS rounds of CALLS calls between two
events; the spread is the fastest and the slowest round.
    python tools/gpu_field_arith_one.py FIELD pointwise|product|quotient LG [LG ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sppark_amd
from sppark_amd import poly
from sppark_amd import NTTInputOutputOrder as Ord, NTTDirection as Dir, NTTType as Typ

field, what = sys.argv[1], sys.argv[2]
lgs = [int(v) for v in sys.argv[3:]]
ROUNDS, WARM = 7, 3
EB = poly._ELEM_BYTES[field]
torch.cuda.set_stream(torch.cuda.Stream())                  # non-null: the pointwise calls and the transforms only enqueue
S = torch.cuda.current_stream().cuda_stream


def column(n, seed, cols=1):
    """cols x n canonical elements of |field| on the device"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    if EB == 8:
        return torch.randint(0, 1 << 62, (cols, n), dtype=torch.int64, device="cuda", generator=g)
    if EB == 4:
        return torch.randint(0, 0x78000001, (cols, n), dtype=torch.int32, device="cuda", generator=g)
    if EB == 16:
        return torch.randint(0, 0x78000001, (cols, n * 4), dtype=torch.int32, device="cuda", generator=g)
    x = torch.randint(0, 1 << 62, (cols, n, 4), dtype=torch.int64, device="cuda", generator=g)      # below 2^252 < every modulus
    x[:, :, 3] &= (1 << 59) - 1
    return x.reshape(cols, n * 4)


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
    """a device-to-device copy of |elements| field elements"""
    src = torch.empty(elements * EB, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
    src.zero_()
    return lambda: dst.copy_(src, non_blocking=True)


print("# %s %s; device %s; lib %s; %d rounds, median [fastest .. slowest] ms per call"
      % (field, what, torch.cuda.get_device_name(0), os.environ.get("SPPARK_LIBDIR", "lib"), ROUNDS), flush=True)
for lg in lgs:
    n = 1 << lg
    calls = 20 if lg <= 22 else 8
    if what == "pointwise":
        a, b, c = (column(n, lg + i)[0] for i in range(3))
        out = torch.empty_like(a)
        k = column(1, 9)[0].cpu().numpy()
        fns = [("add", lambda: poly.vec_add(out, a, b, field=field, stream=S)),
               ("mul", lambda: poly.vec_mul(out, a, b, field=field, stream=S)),
               ("copy1.5", copier(n + n // 2)),
               ("scale", lambda: poly.vec_scale(out, a, k, field=field, stream=S)),
               ("copy1", copier(n)),
               ("mul_sub_k", lambda: poly.vec_mul_sub(out, a, b, c, k=k, field=field, stream=S)),
               ("copy2", copier(2 * n))]
        if EB == 32:
            fns.append(("scan", lambda: poly.prefix_op(out, a, poly.MULTIPLY, field, stream=S)))
        t = timed(fns, calls)
        gbs = lambda name, arrays: arrays * n * EB / t[name][0] / 1e6
        print("  2^%-3d add %s  mul %s  copy of 1.5 arrays %s  add/copy %.3f mul/copy %.3f  (mul %.0f GB/s, copy %.0f GB/s)"
              % (lg, cell(t["add"]), cell(t["mul"]), cell(t["copy1.5"]), t["add"][0] / t["copy1.5"][0], t["mul"][0] / t["copy1.5"][0],
                 gbs("mul", 3), gbs("copy1.5", 3)), flush=True)
        print("        scale %s  copy of 1 array %s  ratio %.3f;  mul_sub(k) %s  copy of 2 arrays %s  ratio %.3f"
              % (cell(t["scale"]), cell(t["copy1"]), t["scale"][0] / t["copy1"][0], cell(t["mul_sub_k"]), cell(t["copy2"]),
                 t["mul_sub_k"][0] / t["copy2"][0]), flush=True)
        if EB == 32:
            print("        prefix_op(MULTIPLY) %s  mul/scan %.3f" % (cell(t["scan"]), t["mul"][0] / t["scan"][0]), flush=True)
    elif what == "product":                                   # la = lb = 2^lg: transforms of 2^(lg + 1)
        a, b = column(n, lg)[0], column(n, lg + 1)[0]
        out = torch.empty((2 * n - 1) * (EB // a.element_size()), dtype=a.dtype, device="cuda")
        x = column(2 * n, lg + 2)[0]
        fns = [("product", lambda: poly.product(out, a, b, field=field, stream=S)),
               ("fwd", lambda: sppark_amd.compute_ntt(0, x, Ord.NR, Dir.Forward, Typ.Standard, field, stream=S)),
               ("inv", lambda: sppark_amd.compute_ntt(0, x, Ord.RN, Dir.Inverse, Typ.Standard, field, stream=S)),
               ("copy", copier(4 * 2 * n))]                 # pad: n read + 2N written; product: 3N; copy-out: 2N (N = 2n): 8N / 2
        t = timed(fns, calls)
        budget = 2 * t["fwd"][0] + t["inv"][0] + t["copy"][0]
        print("  la = lb = 2^%-3d product %s  forward NR %s  inverse RN %s  copy of 4N elements %s  budget %.4f  product/budget %.3f"
              % (lg, cell(t["product"]), cell(t["fwd"]), cell(t["inv"]), cell(t["copy"]), budget, t["product"][0] / budget), flush=True)
    elif what == "quotient":
        abc = column(n, lg, 3)
        a, b, c = abc[0], abc[1], abc[2]
        h = torch.empty_like(a)
        w = column(n, lg + 5, 3)
        fns = [("quotient", lambda: poly.vanishing_quotient(h, a, b, c, field=field, stream=S)),
               ("inv3", lambda: sppark_amd.compute_ntt_batch(0, w, Ord.NR, Dir.Inverse, Typ.Standard, field, stream=S)),
               ("cfwd3", lambda: sppark_amd.compute_ntt_batch(0, w, Ord.RN, Dir.Forward, Typ.Coset, field, stream=S)),
               ("cinv", lambda: sppark_amd.compute_ntt(0, w[0], Ord.NN, Dir.Inverse, Typ.Coset, field, stream=S)),
               ("copy", copier(6 * n))]                     # staging 3n + 3n, mul_sub 3n + n, into h n + n: 12n / 2
        t = timed(fns, calls)
        budget = t["inv3"][0] + t["cfwd3"][0] + t["cinv"][0] + t["copy"][0]
        print("  2^%-3d quotient %s  3 x inverse NR %s  3 x coset forward RN %s  coset inverse NN %s  copy of 6n elements %s  budget %.4f  quotient/budget %.3f"
              % (lg, cell(t["quotient"]), cell(t["inv3"]), cell(t["cfwd3"]), cell(t["cinv"]), cell(t["copy"]), budget,
                 t["quotient"][0] / budget), flush=True)
