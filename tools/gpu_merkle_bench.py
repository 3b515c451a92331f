"""Merkle commitments (sppark_amd.merkle.commit) on device-resident matrices, each shape next to two floors that do not come
from the code under test:

  memory floor  poly.vec_scale (sppark_field_scale, older than the commitments) over the same number of input bytes,
                alternating with the commitment in the same run: one streaming pass that reads them and writes as many
  issue floor   vector instructions per compression, counted in the built code object's disassembly, times the compressions
                of the call, divided by the chip's vector issue rate: CUs x 4 SIMDs x 32 lanes per cycle (a wave64
                instruction takes a SIMD two cycles) at 2.4 GHz

Device buffers, a non-default stream (the calls only enqueue), WARM calls first, then the median of ROUNDS rounds of CALLS calls
between two events; the spread is the fastest and the slowest round.  A result more than 1.5 x above the larger floor is
reported as MISSED.

    python tools/gpu_merkle_bench.py count                  the instruction counts, from build/obj (where the objects are)
    python tools/gpu_merkle_bench.py run B2S_LEAF,B2S_NODE,SHA_LEAF,SHA_NODE [small]
                                                            the measurement, with the counts of the first command"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CLOCK_HZ, LANES_PER_SIMD_CYCLE, SIMDS = 2.4e9, 32, 4
ROUNDS, WARM = 7, 3


def count():
    """VALU instructions of the leaves kernel (one 64-byte block per trip of its loop; its prologue and epilogue counted in)
    and of the nodes kernel divided by its seven nodes, per hash, from the gl64 library's object"""
    import isa_stats
    co = isa_stats.code_object(os.path.join(ROOT, "build", "obj", "gl64__api_ntt_api.hip.o"))
    txt = subprocess.run([isa_stats.LLVM + "/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    valu, name = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
        elif name and re.match(r"^\s+v_", line):
            valu[name] = valu.get(name, 0) + 1
    pick = lambda word: [v for k, v in valu.items() if re.search(word, k)]                   # noqa: E731
    out = []
    for h in (0, 1):
        leaf = pick(r"k_merkle_leavesILj2ELi%dELb1E" % h)
        node = pick(r"k_merkle_nodesILi%dELj3E" % h)
        assert len(leaf) == 1 and len(node) == 1, (leaf, node)
        out += [leaf[0], -(-node[0] // 7)]
    print("VALU instructions: BLAKE2s leaf block %d, node %d; SHA-256 leaf block %d, node (a block and the constant padding block) %d"
          % tuple(out))
    print(",".join(str(v) for v in out))


def run(counts, small):
    import torch
    from sppark_amd import merkle, poly
    torch.cuda.set_stream(torch.cuda.Stream())
    S = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue_rate = cus * SIMDS * LANES_PER_SIMD_CYCLE * CLOCK_HZ                              # lane-instructions per second
    valu = {"blake2s": counts[0:2], "sha256": counts[2:4]}

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

    def blocks(hash, leaf_bytes):                                                           # noqa: A002
        return max(1, -(-leaf_bytes // 64)) if hash == "blake2s" else (leaf_bytes + 9 + 63) // 64

    print("# device %s, %d CUs; %d rounds, median [fastest .. slowest] ms per call; issue rate %.1f T lane-instructions/s"
          % (torch.cuda.get_device_name(0), cus, ROUNDS, issue_rate / 1e12), flush=True)
    shift = 6 if small else 0
    shapes = [("bb31", 22 - shift, 64, "columns"), ("gl64", 22 - shift, 32, "columns"), ("bls12_381", 22 - shift, 1, "columns"),
              ("m31", 24 - shift, 1, "columns"), ("bb31", 22 - shift, 64, "rows")]
    for field, lg, width, layout in shapes:
        eb = poly._ELEM_BYTES[field]
        n = 1 << lg
        words = eb // 4
        g = torch.Generator(device="cuda"); g.manual_seed(lg + width)
        lines, count_ = (width, n) if layout == "columns" else (n, width)
        mat = torch.randint(0, 0x78000001, (lines, count_ * words), dtype=torch.int32, device="cuda", generator=g)
        if eb == 32:
            mat[:, 7::8] &= 0x0fffffff                                                      # below every modulus
        flat = mat.reshape(-1)
        out = torch.empty_like(flat)
        k = flat[:words].cpu().numpy().copy()
        tree = torch.empty(merkle.tree_bytes(lg), dtype=torch.uint8, device="cuda")
        in_bytes = n * width * eb
        calls = 10 if in_bytes <= (1 << 28) else 4
        fns = [("scale", lambda: poly.vec_scale(out, flat, k, field=field, stream=S))]
        for h in ("blake2s", "sha256"):
            fns.append((h, lambda h=h: merkle.commit(mat, hash=h, layout=layout, field=field, tree=tree, stream=S)))
        t = timed(fns, calls)
        for h in ("blake2s", "sha256"):
            leaf_v, node_v = valu[h]
            nb = blocks(h, width * eb)
            issue_ms = (n * nb * leaf_v + (n - 1) * node_v) / issue_rate * 1e3
            mem_ms = t["scale"][0]
            floor, which = max((issue_ms, "issue"), (mem_ms, "memory"))
            ratio = t[h][0] / floor
            print("  %-9s 2^%d x %-2d %-7s %-7s %.4f [%.4f .. %.4f] ms  %7.1f GB/s of leaves;  vec_scale over the same bytes %.4f [%.4f .. %.4f];"
                  "  issue floor %.4f (%d blocks per leaf);  %s floor binds, ratio %.2f: %s"
                  % (field, lg, width, layout, h, t[h][0], t[h][1], t[h][2], in_bytes / t[h][0] / 1e6, mem_ms, t["scale"][1], t["scale"][2],
                     issue_ms, nb, which, ratio, "met" if ratio <= 1.5 else "MISSED"), flush=True)
        del mat, flat, out, tree


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "count":
        count()
    elif len(sys.argv) >= 3 and sys.argv[1] == "run":
        run([int(v) for v in sys.argv[2].split(",")], len(sys.argv) > 3 and sys.argv[3] == "small")
    else:
        sys.exit(__doc__)
