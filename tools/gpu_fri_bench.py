"""FRI calls (sppark_amd.fri) on device-resident vectors, each next to a yardstick that is not the code under test and runs
alternating with it in the same run:

  fold, arity 1, 2^24   mle.fold of the same table (older than the fold; moves the same bytes: n read, n / 2 written).
                        NATURAL pairs are mle's HIGH, BITREV pairs mle's LOW.  For elements of 4 and 8 bytes the target is
                        parity, the margin mle.fold's own fastest-to-slowest spread in the run; for 16 and 32 bytes the
                        ratio is reported with the kernel's static vector-instruction count per result.
  fold, arity 3         three arity-1 calls (n, n / 2, n / 4) and the share of their traffic it moves:
                        (1 + 1/8) / (3/2 + 3/4 + 3/8) = 3/7 by bytes (7/12 if only the reads of the three calls are counted
                        against its read and write).
  reduce                a bb31 matrix 2^22 x 64 into bb31x4, both layouts: poly.vec_scale over the same number of input
                        bytes (it reads them AND writes as many: twice the traffic).  The issue floor comes from `count`:
                        the instructions of the kernel's main loop (four loads, sixteen matrix elements per lane) at the
                        rates this project measured on the chip with eight waves per SIMD
                        (profiles/r02_ubench_instruction_rates.log): 0.205 wave-instructions per clock and SIMD for
                        v_mad_u64_u32, 0.338 for a 32-bit vector instruction; 256 CUs x 4 SIMDs at 2.4 GHz.

Device buffers, a non-default stream (the calls only enqueue), WARM calls first, then the median of ROUNDS rounds of CALLS calls
between two events; the spread is the fastest and the slowest round.

    python tools/gpu_fri_bench.py count            static instruction counts, from build/obj (where the objects are)
    python tools/gpu_fri_bench.py run [small]      the measurement"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLOCK_HZ, LANES_PER_SIMD_CYCLE, SIMDS = 2.4e9, 32, 4
ROUNDS, WARM = 7, 3
OBJECTS = {"gl64": "gl64__api_ntt_api.hip.o", "bb31": "bb31__api_ntt_api.hip.o", "bb31x4": "bb31x4__api_poly_only_api.hip.o",
           "bls12_381": "bls12_381__api_ntt_api.hip__SPPARK_NTT_WITH_MSM.o"}
# results per lane and tile of the arity-1 fold with 16-byte accesses (csrc/fri/fri_route.hpp)
FOLD1_PER_LANE = {"gl64": 4, "bb31": 8, "bb31x4": 2, "bls12_381": 1}


def _valu(obj):
    """{demangled kernel name: static VALU / all instructions} of one object"""
    import isa_stats
    co = isa_stats.code_object(os.path.join(ROOT, "build", "obj", obj))
    txt = subprocess.run([isa_stats.LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    out, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            out[name] = [0, 0]
        elif name and re.match(r"^\s+[a-z]", line):
            out[name][1] += 1
            if re.match(r"^\s+v_", line):
                out[name][0] += 1
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {d: tuple(out[n]) for n, d in zip(names, dem)}


MAD_RATE, VALU_RATE, CUS = 0.205, 0.338, 256        # wave-instructions per clock and SIMD (r02_ubench_instruction_rates.log)


def _reduce_loops():
    """the main loop of the two bb31 -> bb31x4 reduce kernels (16-byte accesses): the backward branch whose body holds
    FRI_LAZY_TERMS = 4 global loads; 16 matrix elements per lane and trip"""
    import isa_stats
    co = isa_stats.code_object(os.path.join(ROOT, "build", "obj", OBJECTS["bb31x4"]))
    txt = subprocess.run([isa_stats.LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    kernels, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1); kernels[name] = []
            continue
        m = re.match(r"^\s+(\S+).*//\s*([0-9A-Fa-f]+):(.*)$", line)
        if m and name:
            kernels[name].append((int(m.group(2), 16), m.group(1), m.group(3)))
    names = list(kernels)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    for n, d in zip(names, dem):
        m = re.search(r"k_fri_reduce<.*bb31_4_dev, .*bb31_dev, (true|false), true>", d)
        if not m:
            continue
        ins = kernels[n]
        for a, op, tail in ins:
            t = re.search(r"<\S+\+0x([0-9a-f]+)>", tail)
            if not (op.startswith("s_cbranch") or op == "s_branch") or not t or ins[0][0] + int(t.group(1), 16) > a:
                continue
            body = [x for x in ins if ins[0][0] + int(t.group(1), 16) <= x[0] <= a]
            loads = sum(1 for x in body if x[1].startswith("global_load"))
            if loads != 4:
                continue
            mad = sum(1 for x in body if x[1].startswith("v_mad_u64_u32"))
            valu = sum(1 for x in body if x[1].startswith("v_"))
            clk = mad / MAD_RATE + (valu - mad) / VALU_RATE                                   # per wave and trip, on one SIMD
            ms = (1 << 28) / (64 * 16) * clk / (CUS * 4) / CLOCK_HZ * 1e3
            print("bb31x4     k_fri_reduce bb31 -> bb31x4, %-7s main loop: %d instructions, VALU %d of which v_mad_u64_u32 %d, for 16 elements"
                  " per lane = %.1f VALU per element;  issue floor for 2^22 x 64 at the measured rates: %.3f ms"
                  % ("columns" if m.group(1) == "true" else "rows", len(body), valu, mad, valu / 16, ms))
            break


def count():
    _reduce_loops()
    for field, obj in OBJECTS.items():
        k = _valu(obj)
        for name, (valu, total) in sorted(k.items()):
            if "k_fri_" not in name:
                continue
            short = re.sub(r"sppark_amd::|\(.*", "", name)
            note = ""
            if "k_fri_fold" in short and ", 1u, " in short and short.rstrip(">").endswith("true"):
                note = "   = %.0f VALU per result if a lane took one tile (prologue included)" % (valu / FOLD1_PER_LANE[field])
            print("%-10s %-78s VALU %5d of %5d%s" % (field, short[:78], valu, total, note))


def run(small):
    import numpy as np
    import torch
    from sppark_amd import fri, mle, poly
    torch.cuda.set_stream(torch.cuda.Stream())
    S = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue_rate = cus * SIMDS * LANES_PER_SIMD_CYCLE * CLOCK_HZ

    def timed(fns, calls):
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

    def vector(field, n, seed):
        words = poly._ELEM_BYTES[field] // 4
        g = torch.Generator(device="cuda"); g.manual_seed(seed)
        t = torch.randint(0, 0x78000001, (n, words), dtype=torch.int32, device="cuda", generator=g)
        if words == 8:
            t[:, 7] &= 0x0fffffff                                                           # below every modulus
        return t

    fmt = lambda t: "%.4f [%.4f .. %.4f]" % t                                                # noqa: E731
    print("# device %s, %d CUs; %d rounds, median [fastest .. slowest] ms per call" % (torch.cuda.get_device_name(0), cus, ROUNDS), flush=True)
    lg = 18 if small else 24
    n = 1 << lg
    print("# fold, arity 1, 2^%d elements, against mle.fold of the same table" % lg)
    for field in ("bb31", "gl64", "bb31x4", "bls12_381"):
        eb = poly._ELEM_BYTES[field]
        x = vector(field, n, lg)
        out = torch.empty_like(x[:n // 2])
        beta = x[:1].clone()
        for order, mle_order, name in ((fri.NATURAL, mle.HIGH, "NATURAL"), (fri.BITREV, mle.LOW, "BITREV")):
            t = timed([("mle", lambda: mle.fold(out, x, beta, order=mle_order, field=field, stream=S)),
                       ("fri", lambda: fri.fold(out, x, beta, lg_arity=1, order=order, field=field, stream=S))], 10)
            ratio = t["fri"][0] / t["mle"][0]
            verdict = ""
            if eb <= 8:
                verdict = ";  parity within mle.fold's spread: " + ("met" if t["fri"][0] <= t["mle"][0] + (t["mle"][2] - t["mle"][1]) else "MISSED")
            print("  %-9s %-7s fri.fold %s ms  %7.1f GB/s;  mle.fold %s;  ratio %.3f%s"
                  % (field, name, fmt(t["fri"]), 1.5 * n * eb / t["fri"][0] / 1e6, fmt(t["mle"]), ratio, verdict), flush=True)
        # arity 3 against three arity-1 calls
        o1, o2, o3 = torch.empty_like(x[:n // 2]), torch.empty_like(x[:n // 4]), torch.empty_like(x[:n // 8])
        for order, name in ((fri.NATURAL, "NATURAL"), (fri.BITREV, "BITREV")):
            def three():
                fri.fold(o1, x, beta, lg_arity=1, order=order, field=field, stream=S)
                fri.fold(o2, o1, beta, lg_arity=1, order=order, field=field, stream=S)
                fri.fold(o3, o2, beta, lg_arity=1, order=order, field=field, stream=S)
            t = timed([("three", three), ("one", lambda: fri.fold(o3, x, beta, lg_arity=3, order=order, field=field, stream=S))], 10)
            print("  %-9s %-7s arity 3 %s ms  %7.1f GB/s;  three arity-1 calls %s;  ratio %.3f (traffic 3/7 = 0.429)"
                  % (field, name, fmt(t["one"]), 1.125 * n * eb / t["one"][0] / 1e6, fmt(t["three"]), t["one"][0] / t["three"][0]), flush=True)
        del x, out, o1, o2, o3

    lg, width = (16 if small else 22), 64
    n = 1 << lg
    print("# reduce, bb31 matrix 2^%d x %d into bb31x4" % (lg, width))
    w = vector("bb31x4", width, 5)
    out = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    for layout in ("columns", "rows"):
        mat = vector("bb31", n * width, 7).reshape((width, n) if layout == "columns" else (n, width))
        flat = mat.reshape(-1)
        sink = torch.empty_like(flat)
        k = flat[:1].cpu().numpy().copy()
        t = timed([("scale", lambda: poly.vec_scale(sink, flat, k, field="bb31", stream=S)),
                   ("reduce", lambda: fri.reduce(out, mat, w, layout=layout, base=True, field="bb31x4", stream=S))], 4)
        in_bytes = n * width * 4
        print("  %-7s fri.reduce %s ms  %7.1f GB/s of matrix;  vec_scale over the same bytes (read and written) %s  %7.1f GB/s of traffic"
              % (layout, fmt(t["reduce"]), in_bytes / t["reduce"][0] / 1e6, fmt(t["scale"]), 2 * in_bytes / t["scale"][0] / 1e6), flush=True)
        del mat, flat, sink


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "count":
        count()
    elif len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(len(sys.argv) > 2 and sys.argv[2] == "small")
    else:
        sys.exit(__doc__)
