"""CPU: register / scratch budgets of the batched NTT's kernels, read from the objects the build left under build/obj
(tools/isa_stats.py, as tests/test_build_resources.py).

k_ntt_small_packed (columns of 2^1 ... 2^6 elements, 256-lane work-groups) is planned for eight waves per SIMD on the
single-word fields (<= 64 registers) and three on the 256-bit ones (<= 168), with no scratch.  Giving every launch of the
plan a column dimension (blockIdx.y, a size_t column offset) must not cost the single transforms registers: the largest
register count of each kernel family below is the one it had before the batched entry points (the offset is a scalar
multiply-add per work-group: VALU counts unchanged, DESIGN.md "Batched transforms")."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OBJ = os.path.join(ROOT, "build", "obj")
FAMILIES = {"k_ntt6": "6k_ntt6I", "k_ntt12": "7k_ntt12I", "k_ntt_small": "11k_ntt_smallI", "k_ntt_pass": "10k_ntt_passI",
            "k_ntt_pass_lat": "14k_ntt_pass_latI", "k_ntt_small_packed": "18k_ntt_small_packedI"}


def _families(obj):
    import isa_stats
    path = os.path.join(OBJ, obj)
    if not os.path.exists(path):
        pytest.skip("%s not built here" % obj)
    out = {}
    for sym, md in isa_stats.metadata(isa_stats.code_object(path)).items():
        if "vgpr_count" not in md:
            continue
        for fam, tag in FAMILIES.items():
            if tag in sym:
                regs = int(md.get("vgpr_count") or 0) + int(md.get("agpr_count") or 0)
                scratch = int(md.get("private_segment_fixed_size") or 0)
                r, s = out.get(fam, (0, 0))
                out[fam] = (max(r, regs), max(s, scratch))
    return out


# (largest registers, largest scratch bytes) per family, measured on the objects of the tree before the batched entry points
BEFORE = {
    "gl64__ntt_k_ntt_r64.hip__SPPARK_NTT_DIF=0.o": {"k_ntt6": (64, 0), "k_ntt12": (64, 0)},
    "gl64__ntt_k_ntt_r64.hip__SPPARK_NTT_DIF=1.o": {"k_ntt6": (59, 0), "k_ntt12": (62, 0)},
    "gl64__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o": {"k_ntt_pass": (116, 0)},
    "gl64__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=1.o": {"k_ntt_pass": (102, 0), "k_ntt_small": (55, 0)},
    "bb31__ntt_k_ntt_r64.hip__SPPARK_NTT_DIF=0.o": {"k_ntt6": (27, 0), "k_ntt12": (29, 0)},
    "bb31__ntt_k_ntt_r64.hip__SPPARK_NTT_DIF=1.o": {"k_ntt6": (26, 0), "k_ntt12": (31, 0)},
    "bb31__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o": {"k_ntt_pass": (60, 0)},
    "bb31__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=1.o": {"k_ntt_pass": (64, 0), "k_ntt_small": (37, 0)},
    "bls12_381__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o": {"k_ntt_pass": (97, 144), "k_ntt_pass_lat": (75, 0)},
    "bls12_381__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=1.o": {"k_ntt_pass": (88, 144), "k_ntt_small": (156, 0), "k_ntt_pass_lat": (68, 0)},
}


@pytest.mark.parametrize("obj", sorted(BEFORE))
def test_single_transform_kernels_keep_their_registers(obj):
    now = _families(obj)
    for fam, (regs, scratch) in BEFORE[obj].items():
        assert fam in now, (obj, fam)
        assert now[fam][0] <= regs and now[fam][1] <= scratch, (obj, fam, now[fam], (regs, scratch))


@pytest.mark.parametrize("obj,max_regs", [("gl64__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o", 64), ("bb31__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o", 64),
                                          ("bls12_381__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o", 168),
                                          ("bn254__ntt_k_ntt_pass.hip__SPPARK_NTT_DIF=0.o", 168)])
def test_packed_kernel_budget(obj, max_regs):
    now = _families(obj)
    assert "k_ntt_small_packed" in now, obj
    regs, scratch = now["k_ntt_small_packed"]
    assert regs <= max_regs and scratch == 0, (obj, regs, scratch)
