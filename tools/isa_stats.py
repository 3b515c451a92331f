"""Per-kernel ISA statistics of a compiled translation unit (no GPU needed).

    python tools/isa_stats.py build/obj/<unit>.o [kernel-name-substring] [--classes] [--dump]

Extracts the gfx950 code object from the object's .hip_fatbin, prints for every kernel (or those
whose demangled name contains the substring) the register / LDS / scratch figures of the kernel
descriptor's metadata and a STATIC count of its instructions by opcode (straight-line count of the
emitted code, loops counted once).  --classes groups the opcodes the way DESIGN.md's instruction
accounts do; --dump writes the disassembly of the selected kernels to stdout.

    python tools/isa_stats.py <unit>.s [kernel-name-substring] --waits

reads the ASSEMBLY hipcc writes with --cuda-device-only -S (it keeps the block labels and the loop each block belongs to,
which a disassembly does not) and lists, for the main loop of every selected kernel, its vector-memory instructions and
its `s_waitcnt vmcnt` in program order: where a wave can be parked on memory.  asm_kernels() / main_loop() / loop_waits()
are what tests/test_accumulate_waits.py asserts on.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"

CLASSES = [
    ("v_mad_u64_u32", "multiply-add 32x32+64"),
    ("v_mul_lo_u32", "multiply (low)"), ("v_mul_hi_u32", "multiply (high)"), ("v_mul_u32_u24", "multiply 24"),
    ("v_lshrrev_b64", "64-bit shift"), ("v_lshlrev_b64", "64-bit shift"), ("v_lshl_add_u64", "64-bit add"),
    ("v_add_co_u32", "carry add/sub"), ("v_addc_co_u32", "carry add/sub"), ("v_sub_co_u32", "carry add/sub"),
    ("v_subb_co_u32", "carry add/sub"), ("v_subbrev_co_u32", "carry add/sub"), ("v_subrev_co_u32", "carry add/sub"),
    ("v_and_b32", "mask / logic"), ("v_or_b32", "mask / logic"), ("v_xor_b32", "mask / logic"), ("v_not_b32", "mask / logic"),
    ("v_and_or_b32", "mask / logic"), ("v_bfe_u32", "mask / logic"), ("v_bfi_b32", "mask / logic"), ("v_or3_b32", "mask / logic"),
    ("v_lshrrev_b32", "32-bit shift"), ("v_lshlrev_b32", "32-bit shift"), ("v_alignbit_b32", "32-bit shift"),
    ("v_lshl_or_b32", "32-bit shift"), ("v_lshl_add_u32", "32-bit shift"), ("v_ashrrev_i32", "32-bit shift"),
    ("v_add_u32", "32-bit add/sub"), ("v_sub_u32", "32-bit add/sub"), ("v_subrev_u32", "32-bit add/sub"),
    ("v_add3_u32", "32-bit add/sub"), ("v_add_lshl_u32", "32-bit add/sub"),
    ("v_mov_b32", "move"), ("v_accvgpr_write_b32", "move"), ("v_accvgpr_read_b32", "move"), ("v_pk_mov_b32", "move"),
    ("v_mov_b64", "move"),
    ("v_cndmask_b32", "select"), ("v_cmp", "compare"), ("v_readfirstlane_b32", "lane op"), ("v_readlane_b32", "lane op"),
]


def klass(op):
    for prefix, name in CLASSES:
        if op.startswith(prefix):
            return name
    if op.startswith("v_"):
        return "other VALU"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_"):
        return "SALU / branch"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM (" + ("scratch" if op.startswith("scratch_") else "global") + ")"
    return "other"


def code_object(path):
    tmp = tempfile.mkdtemp(prefix="isa_")
    if open(path, "rb").read(4) == b"\x7fELF":
        sections = subprocess.run([LLVM + "/llvm-readelf", "-S", path], capture_output=True, text=True).stdout
        if ".hip_fatbin" not in sections:
            return path                                         # already a device code object
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path])
    else:
        fat = path
    co = os.path.join(tmp, "dev.co")
    subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def metadata(co):
    """{kernel symbol: {field: value}} from the amdhsa.kernels metadata note (one '- .agpr_count' list item per kernel)"""
    txt = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    out, cur = {}, None
    keep = ("agpr_count", "vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
            "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size", "symbol")
    for line in txt.splitlines():
        m = re.match(r"^(\s+)(- )?\.(\w+):\s+(.*)", line)
        if not m:
            continue
        indent, item, k, v = len(m.group(1)), m.group(2), m.group(3), m.group(4).strip().strip("'")
        if item and indent == 2:                                # a new kernel record (top-level list item)
            if cur and "symbol" in cur:
                out[cur["symbol"].replace(".kd", "")] = cur
            cur = {}
        if cur is not None and indent <= 4 and k in keep:
            cur[k] = v
    if cur and "symbol" in cur:
        out[cur["symbol"].replace(".kd", "")] = cur
    return out


def asm_kernels(path):
    """{symbol: {"ins": [...], "NumVgprs": n, "ScratchSize": n, "Occupancy": n}} of an assembly file (hipcc -S).  One entry of
    "ins" per instruction: {"op", "args", "block": label of its basic block, "loop": header label of the OUTERMOST loop the
    block is in (None outside loops), "depth": loop depth of the block}."""
    out, cur, sym = collections.OrderedDict(), None, None
    block, loop, depth = None, None, 0
    for line in open(path):
        line = line.rstrip("\n")
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(?:;.*)?$", line)
        if m and not m.group(1).startswith((".L", "__hip")):                # a function's entry label
            sym = m.group(1)
            cur = out[sym] = {"ins": []}
            block, loop, depth = sym, None, 0
            continue
        if cur is None:
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m:
            out[sym][m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"^(\.LBB\d+_\d+):\s*(?:;\s*(.*))?$", line) or re.match(r"^; %bb\.(\d+):\s*(?:;\s*(.*))?$", line)
        if m:
            block, note = m.group(1), m.group(2) or ""
            # "=>This Loop Header: Depth=1" | "in Loop: Header=BB0_25 Depth=1" | "Parent Loop BB0_25 Depth=1" (+ a line
            # "=>  This Inner Loop Header: Depth=2" below it) | nothing: not in a loop
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            if "This Loop Header" in note:
                loop, depth = block.replace(".L", ""), 1
            elif h:
                depth = int(h.group(2))
                loop = h.group(1) if depth == 1 else loop
            elif "Parent Loop" in note:
                loop, depth = re.search(r"Parent Loop (BB\d+_\d+)", note).group(1), 2
            else:
                loop, depth = None, 0
            continue
        m = re.match(r"^\s+;\s+=>\s*This Inner Loop Header: Depth=(\d+)", line)
        if m:
            depth = int(m.group(1))
            continue
        m = re.match(r"^\t([a-z]\w*)\b\s*(.*?)\s*(?:;.*)?$", line)
        if m and sym in out and "Occupancy" not in out[sym]:
            cur["ins"].append({"op": m.group(1), "args": m.group(2), "block": block, "loop": loop, "depth": depth})
    return out


def main_loop(kernel):
    """the instructions of the kernel's largest outermost loop, in program order (inner loops included: depth 2 and more)"""
    size = collections.Counter(i["loop"] for i in kernel["ins"] if i["loop"])
    if not size:
        return []
    top = size.most_common(1)[0][0]
    return [i for i in kernel["ins"] if i["loop"] == top]


def is_vmem(op):
    return op.startswith(("global_", "buffer_", "flat_", "scratch_"))


def loop_waits(loop):
    """[(position in the loop, kind, text, depth)] of the loop's vector-memory instructions ("load" / "store"), its
    `s_waitcnt vmcnt` ("wait") and the first v_mad_u64_u32 after each of them ("mad": where arithmetic resumes)"""
    ev, want_mad = [], False
    for k, i in enumerate(loop):
        op, args = i["op"], i["args"]
        if op == "s_waitcnt" and "vmcnt" in args:
            ev.append((k, "wait", "s_waitcnt " + args, i["depth"])); want_mad = True
        elif is_vmem(op):
            ev.append((k, "store" if "store" in op else "load", op + " " + args, i["depth"])); want_mad = True
        elif op == "v_mad_u64_u32" and want_mad:
            ev.append((k, "mad", "v_mad_u64_u32 (arithmetic resumes)", i["depth"])); want_mad = False
    return ev


def print_waits(path, want):
    for sym, kern in asm_kernels(path).items():
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        if (want and want not in dem and want not in sym) or "NumVgprs" not in kern:
            continue
        loop = main_loop(kern)
        ops = collections.Counter(i["op"] for i in kern["ins"])
        print("== %s" % dem[:160])
        print("   vgpr %s  scratch %s B  waves/SIMD %s  v_mad_u64_u32 %d  |  main loop: %d instructions, %d v_mov_b64, %d s_waitcnt vmcnt"
              % (kern.get("NumVgprs"), kern.get("ScratchSize"), kern.get("Occupancy"), ops["v_mad_u64_u32"], len(loop),
                 sum(i["op"].startswith("v_mov_b64") for i in loop), sum(i["op"] == "s_waitcnt" and "vmcnt" in i["args"] for i in loop)))
        run = None
        for k, kind, text, depth in loop_waits(loop) + [(None, None, None, None)]:
            # runs of alike loads / stores on one line
            head = text.split(" ")[0] if kind in ("load", "store") else None
            if run and (head != run[1] or depth != run[3]):
                print("   %6d  %s%s%s" % (run[0], "    " * (run[3] - 1), run[1], "  x %d" % run[2] if run[2] > 1 else ""))
                run = None
            if kind in ("load", "store"):
                run = [k, head, 1, depth] if run is None else [run[0], run[1], run[2] + 1, depth]
            elif kind:
                print("   %6d  %s%s" % (k, "    " * (depth - 1), text))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0]
    want = args[1] if len(args) > 1 else ""
    if "--waits" in sys.argv:
        return print_waits(path, want)
    co = code_object(path)
    meta = metadata(co)
    dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    kernels, cur = collections.OrderedDict(), None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1); kernels[cur] = []; continue
        if cur is None:
            continue
        m = re.match(r"^\s+(\w+)\b(.*?)(?://.*)?$", line)
        if m and not line.lstrip().startswith("//"):
            kernels[cur].append((m.group(1), m.group(2)))
    for sym, ins in kernels.items():
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        if want and want not in dem and want not in sym:
            continue
        md = meta.get(sym, {})
        print("== %s" % dem[:200])
        if md:
            print("   vgpr %s  agpr %s  sgpr %s  lds %s B  scratch %s B  vgpr spills %s" % (
                md.get("vgpr_count"), md.get("agpr_count"), md.get("sgpr_count"), md.get("group_segment_fixed_size"),
                md.get("private_segment_fixed_size"), md.get("vgpr_spill_count")))
        if "--dump" in sys.argv:
            for op, rest in ins:
                print("      %s%s" % (op, rest))
            continue
        cnt = collections.Counter(op for op, _ in ins)
        valu = sum(v for k, v in cnt.items() if k.startswith("v_"))
        print("   %d instructions, %d VALU" % (len(ins), valu))
        if "--classes" in sys.argv:
            cc = collections.Counter()
            for op, v in cnt.items():
                cc[klass(op)] += v
            for k, v in cc.most_common():
                print("   %8d  %s" % (v, k))
        else:
            for k, v in cnt.most_common(40):
                print("   %8d  %s" % (v, k))


if __name__ == "__main__":
    main()
