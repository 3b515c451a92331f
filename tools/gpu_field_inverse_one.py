"""Field-vector inverse and quotient on device-resident arrays: time per call of poly.inverse and poly.divide next to
poly.prefix_op(MULTIPLY) -- the same three launches and the same 2 reads + 1 write of the array -- in the same run.
Each figure is the median of ROUNDS rounds of CALLS calls (the three operations alternate inside a round); the spread is
the fastest and the slowest round.  --host adds, once, what the calls replace at 2^20: copy the column out, invert it on
the host (Python's pow, element by element), copy it back.
    python tools/gpu_field_inverse_one.py [field] [--host]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, sppark_amd
from sppark_amd import poly

field = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "gl64"
ROUNDS, CALLS, WARM = 7, 20, 3
MOD = {"gl64": 0xffffffff00000001, "gl64_plonky2": 0xffffffff00000001, "bb31": 0x78000001, "bb31_canonical": 0x78000001, "m31": 0x7fffffff}


def column(n, seed):
    """n canonical non-zero elements of |field| on the device"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    if field in ("gl64", "gl64_plonky2"):
        return torch.randint(1, 1 << 62, (n,), dtype=torch.int64, device="cuda", generator=g)
    if field in ("bb31", "bb31_canonical", "m31"):
        return torch.randint(1, MOD[field], (n,), dtype=torch.int32, device="cuda", generator=g)
    if field == "bb31x4":
        return torch.randint(1, 0x78000001, (n, 4), dtype=torch.int32, device="cuda", generator=g)
    x = torch.randint(1, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)      # 256-bit: below 2^252 < every modulus
    x[:, 3] &= (1 << 59) - 1
    return x


print("# %s; device %s; %d rounds x %d calls, median [fastest .. slowest] ms per call" % (field, torch.cuda.get_device_name(0), ROUNDS, CALLS))
print("# %-6s %-28s %-28s %-28s %8s %8s" % ("size", "prefix_op(MULTIPLY)", "inverse", "divide", "inv/scan", "div/scan"))
for lg in (12, 16, 20, 24):
    n = 1 << lg
    x, y = column(n, lg), column(n, 100 + lg)
    out = torch.empty_like(x)
    ops = (("scan", lambda: poly.prefix_op(out, x, poly.MULTIPLY, field)),
           ("inverse", lambda: poly.inverse(out, x, field)),
           ("divide", lambda: poly.divide(out, y, x, field)))
    for _, fn in ops:
        for _ in range(WARM): fn()
    ms = {name: [] for name, _ in ops}
    for _ in range(ROUNDS):
        for name, fn in ops:
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS): fn()
            e1.record(); torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / CALLS)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    cell = {k: "%.4f [%.4f .. %.4f]" % (med[k], min(v), max(v)) for k, v in ms.items()}
    print("  2^%-4d %-28s %-28s %-28s %8.2f %8.2f" % (lg, cell["scan"], cell["inverse"], cell["divide"],
                                                      med["inverse"] / med["scan"], med["divide"] / med["scan"]), flush=True)

if "--host" in sys.argv and field in MOD:
    n, p = 1 << 20, MOD[field]
    x = column(n, 7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = x.cpu().numpy()
    t1 = time.perf_counter()
    if field.startswith("bb31"):
        inv = [pow(int(v), -1, p) * (1 << 64) % p for v in h]          # Montgomery words, R = 2^32
    else:
        inv = [pow(int(v), -1, p) for v in h]
    t2 = time.perf_counter()
    back = torch.tensor(inv, dtype=torch.int64).to(x.dtype).cuda() if x.dtype == torch.int32 else \
        torch.from_numpy(__import__("numpy").array(inv, dtype="uint64").view("int64")).cuda()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    out = torch.empty_like(x)
    poly.inverse(out, x, field)
    assert bool((out == back).all()), "host and device inverses differ"
    print("# host alternative at 2^20: copy out %.2f ms + Python pow() per element %.1f ms + copy back %.2f ms = %.1f ms (same values as poly.inverse)"
          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3), flush=True)
