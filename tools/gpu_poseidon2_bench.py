"""Poseidon2 (sppark_amd.poseidon2.commit / permute) on device-resident data, with the usual parameters (RF = 8, RP = 13 for
BabyBear-16, RP = 22 for Goldilocks-8) and this project's test constants, each shape next to a floor that does not come from
the code under test:

  issue floor   field multiplications per permutation, 4 (RF T + RP) for the S-boxes plus RP T for the diagonal, times the
                vector instructions of ONE bb31_dev / gl64_dev product -- counted in a kernel older than Poseidon2, k_vec of
                poly/vec_kernels.hpp: (a b - c) k has exactly one product more per element than a b - c, so the difference of
                the two instances' VALU counts over the products they hold is one product -- times the permutations of the call,
                divided by the integer issue rate this project measured (profiles/r02_ubench_instruction_rates.log: v_add_u32 at
                eight waves per SIMD, 0.338 wave-instructions per clock and SIMD): CUs x 4 SIMDs x 0.338 x 64 lanes x 2.4 GHz

A result within 1.5 x of the floor is MET, else MISSED.  Also printed: the VALU instructions per permutation of the code
under test (k_p2_permute's disassembly: the body outside the round loops once, each round loop times its trip count), and the
ratio to a BLAKE2s merkle.commit of the same matrix in the same run (recorded, not judged).

Device buffers, a non-default stream (the calls only enqueue), WARM calls first, then the median of ROUNDS rounds of CALLS calls
between two events; the spread is the fastest and the slowest round.

    python tools/gpu_poseidon2_bench.py count               the instruction counts, from build/obj (where the objects are)
    python tools/gpu_poseidon2_bench.py run BB_PRODUCT,GL_PRODUCT,BB_PERM,GL_PERM [small]
                                                            the measurement, with the counts of the first command"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLOCK_HZ, SIMDS, LANES, MEASURED_RATE = 2.4e9, 4, 64, 0.338          # (wave-instructions per clock and SIMD, v_add_u32, 8 waves)
ROUNDS, WARM = 7, 3
USUAL = {"bb31": (16, 8, 13), "gl64": (8, 8, 22)}                    # T, RF, RP


def mults(field):
    t, rf, rp = USUAL[field]
    return 4 * (rf * t + rp) + rp * t


def _kernels(obj):
    """{kernel: [(offset, mnemonic, branch target offset or None)]} of a code object"""
    import isa_stats
    co = isa_stats.code_object(os.path.join(ROOT, "build", "obj", obj))
    txt = subprocess.run([isa_stats.LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, name, start = {}, None, None
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            name, start = m.group(2), int(m.group(1), 16)
            out[name] = []
            continue
        m = re.match(r"^\s+(\w+).*//\s*([0-9A-Fa-f]+):", line)
        if name and m:
            tgt = re.search(r"<\S+\+0x([0-9a-f]+)>\s*$", line) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
            out[name].append((int(m.group(2), 16) - start, m.group(1), int(tgt.group(1), 16) if tgt else None))
    return out


def product_valu(field):
    """VALU instructions of one product: (k_vec<MUL_SUB_K> - k_vec<MUL_SUB>) / the products an instance holds (two unrolled tiles
    of 16 bytes x 4 accesses per lane and the one-element tail)"""
    ks = _kernels("%s__api_ntt_api.hip.o" % field)
    valu = lambda op: [sum(1 for _, mn, _ in v if mn.startswith("v_")) for k, v in ks.items()       # noqa: E731
                       if re.search(r"5k_vecINS_8%s_devELi%dELb1ELb0E" % (field, op), k)]
    with_k, without = valu(5), valu(4)
    assert len(with_k) == 1 and len(without) == 1, (with_k, without)
    products = 2 * 4 * (16 // (4 if field == "bb31" else 8)) + 1
    assert (with_k[0] - without[0]) % products == 0, (with_k, without, products)
    return (with_k[0] - without[0]) // products


def permutation_valu(field):
    """VALU instructions of one permutation in k_p2_permute: the grid-stride loop's body outside the three round loops once
    (load, first M_E, store), the round loops times RF / 2, RP and RF / 2"""
    t, rf, rp = USUAL[field]
    ks = _kernels("%s__api_ntt_api.hip.o" % field)
    ins = [v for k, v in ks.items() if "k_p2_permute" in k]
    assert len(ins) == 1
    ins = ins[0]
    loops = sorted({(tgt, off) for off, mn, tgt in ins if tgt is not None and tgt <= off})          # backward branches
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in loops)]  # (holds no other loop)
    outer = [l for l in loops if l not in inner]
    assert len(inner) == 3 and outer and len({l[0] for l in outer}) == 1, (inner, outer)
    lo, hi = outer[0][0], max(l[1] for l in outer)
    count = lambda a, b: sum(1 for off, mn, _ in ins if a <= off <= b and mn.startswith("v_"))        # noqa: E731
    body = [count(a, b) for a, b in inner]
    return count(lo, hi) - sum(body) + (rf // 2) * body[0] + rp * body[1] + (rf // 2) * body[2], body


def count():
    out = [product_valu("bb31"), product_valu("gl64")]
    for f in ("bb31", "gl64"):
        total, body = permutation_valu(f)
        print("%s: %d field multiplications per permutation; k_p2_permute: %d VALU per permutation (round loops: full %d, partial %d, full %d per trip)"
              % (f, mults(f), total, body[0], body[1], body[2]))
        out.append(total)
    print("VALU instructions of one product (k_vec, (a b - c) k against a b - c): bb31_dev %d, gl64_dev %d" % (out[0], out[1]))
    print(",".join(str(v) for v in out))


def run(counts, small):
    import torch
    from sppark_amd import merkle, poseidon2
    torch.cuda.set_stream(torch.cuda.Stream())
    S = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rate = cus * SIMDS * MEASURED_RATE * LANES * CLOCK_HZ                                    # lane-instructions per second
    product = {"bb31": counts[0], "gl64": counts[1]}
    perm_valu = {"bb31": counts[2], "gl64": counts[3]}

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

    def report(what, field, t, perms, blake=None):
        floor = perms * mults(field) * product[field] / rate * 1e3
        ratio = t[0] / floor
        print("  %-28s %.4f [%.4f .. %.4f] ms;  %d permutations, %.1f G permutations/s;  issue floor %.4f ms (%d products x %d VALU);"
              "  code under test %d VALU per permutation;  ratio %.2f: %s%s"
              % (what, t[0], t[1], t[2], perms, perms / t[0] / 1e6, floor, mults(field), product[field], perm_valu[field], ratio,
                 "MET" if ratio <= 1.5 else "MISSED", "" if blake is None else ";  BLAKE2s commit of the same matrix %.4f [%.4f .. %.4f] ms, Poseidon2 / BLAKE2s %.1f"
                 % (blake[0], blake[1], blake[2], t[0] / blake[0])), flush=True)

    print("# device %s, %d CUs; %d rounds, median [fastest .. slowest] ms per call; measured integer issue rate %.1f T lane-instructions/s"
          % (torch.cuda.get_device_name(0), cus, ROUNDS, rate / 1e12), flush=True)
    shift = 6 if small else 0
    for field, lg, width in (("bb31", 22 - shift, 64), ("gl64", 22 - shift, 32), ("bb31", 22 - shift, 8), ("gl64", 22 - shift, 4)):
        t_, rf, rp = USUAL[field]
        prm = poseidon2.test_params(field, rf, rp)
        prm.device(0)
        n, mod = 1 << lg, poseidon2.MODULUS[field]
        g = torch.Generator(device="cuda"); g.manual_seed(lg + width)
        if field == "bb31":
            mat = torch.randint(0, mod, (width, n), dtype=torch.int32, device="cuda", generator=g)
        else:                                                                           # below p: the top 32 bits below 2^32 - 1
            mat = torch.randint(0, (1 << 32) - 1, (width, n), dtype=torch.int64, device="cuda", generator=g) << 32
            mat |= torch.randint(0, 1 << 32, (width, n), dtype=torch.int64, device="cuda", generator=g)
        tree = torch.empty(merkle.tree_bytes(lg), dtype=torch.uint8, device="cuda")
        tree2 = torch.empty_like(tree)
        calls = 10 if n * width <= (1 << 26) else 4
        t = timed([("poseidon2", lambda: poseidon2.commit(mat, prm, tree=tree, stream=S)),
                   ("blake2s", lambda: merkle.commit(mat, hash="blake2s", field=field, tree=tree2, stream=S))], calls)
        perms = n * -(-width // (t_ // 2)) + n - 1
        report("%s commit 2^%d x %d%s" % (field, lg, width, " (the tree alone)" if width == t_ // 2 else ""), field, t["poseidon2"], perms, t["blake2s"])
        del mat, tree, tree2
    for field in ("bb31", "gl64"):
        t_, rf, rp = USUAL[field]
        prm = poseidon2.test_params(field, rf, rp)
        prm.device(0)
        count_ = 1 << (20 - shift)
        mat = torch.zeros((count_, t_), dtype=torch.int32 if field == "bb31" else torch.int64, device="cuda")
        mat[:, 0] = torch.arange(count_, device="cuda")
        out = torch.empty_like(mat)
        t = timed([("permute", lambda: poseidon2.permute(mat, prm, out=out, stream=S))], 10)
        report("%s permute 2^%d states" % (field, 20 - shift), field, t["permute"], count_)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "count":
        count()
    elif len(sys.argv) >= 3 and sys.argv[1] == "run":
        run([int(v) for v in sys.argv[2].split(",")], len(sys.argv) > 3 and sys.argv[3] == "small")
    else:
        sys.exit(__doc__)
