"""CPU: where the main loop of k_accumulate can be parked on memory, read from the assembly hipcc writes for gfx950
(tools/isa_stats.py --waits; no GPU needed).

Why this is a test: the loop is ~20k cycles of arithmetic per entry with two waves per SIMD, so every round trip a wave
waits for in it is a few per cent of the kernel, and nothing in the source shows one.  Until round 8 the prefetch gather
was decoded where it was issued (an `s_waitcnt vmcnt(6)` straight behind its seven loads), and every bucket boundary
loaded the next offset and waited `vmcnt(0)`, for the fourteen stores of the flush as well.  What is asserted, for the
BLS12-381 instantiation (accumulate_chunk, msm/msm_kernels.hpp):

  * no `s_waitcnt vmcnt` between the last load of the prefetch gather and the first multiply-add behind it;
  * the flush path (from its first store to the gather) issues the load of the offset it keeps ahead and has no
    `s_waitcnt vmcnt`, except in the loop over empty buckets (the rare slow path, one loop level deeper);
  * the budgets that a change of this loop has broken before: <= 256 registers, no scratch, two waves per SIMD, and the
    5838 multiply-adds of the arithmetic as it is (an unrolled or duplicated addition shows here)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL = "k_accumulate<sppark_amd::montx_dev<sppark_amd::bls12_381_fp_p, 28>, false>"


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    import isa_stats
    from sppark_amd import build as B
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "k_accumulate.s")
    # the product's own flags (sppark_amd/build.py), the device side only, as assembly
    r = subprocess.run([HIPCC] + B.FLAGS + ["-DFEATURE_BLS12_381", "--cuda-device-only", "-S",
                                          os.path.join(B.CSRC, "msm", "k_accumulate.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    hit = []
    for sym, kern in isa_stats.asm_kernels(out).items():
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout
        if KERNEL in dem:
            hit.append(kern)
    assert len(hit) == 1, len(hit)
    return hit[0]


def _gather(ev):
    """positions (in the event list) of the prefetch gather: the run of >= 7 global_load_dwordx4 outside inner loops"""
    runs, cur = [], []
    for n, (_, kind, text, depth) in enumerate(ev):
        if kind == "load" and text.startswith("global_load_dwordx4") and depth == 1:
            cur.append(n)
        elif kind == "wait" and cur:
            continue                                            # a wait inside the run does not end it: the first test looks for it
        else:
            if cur:
                runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    runs = [r for r in runs if len(r) >= 7]
    assert len(runs) == 1, runs
    return runs[0]


def test_budgets_and_arithmetic_are_unchanged(kernel):
    assert kernel["NumVgprs"] <= 256, kernel["NumVgprs"]
    assert kernel["ScratchSize"] == 0
    assert kernel["Occupancy"] == 2
    assert sum(i["op"] == "v_mad_u64_u32" for i in kernel["ins"]) == 5838


def test_nothing_waits_between_the_prefetch_gather_and_the_addition(kernel):
    import isa_stats
    ev = isa_stats.loop_waits(isa_stats.main_loop(kernel))
    g = _gather(ev)
    inside = [e for e in ev[g[0]:g[-1]] if e[1] == "wait"]
    assert not inside, inside
    behind = ev[g[-1] + 1:]
    mads = [n for n, e in enumerate(behind) if e[1] == "mad"]
    assert mads, "no multiply-add behind the gather: the gather is not in front of the addition"
    waits = [e for e in behind[:mads[0]] if e[1] == "wait"]
    assert not waits, waits


def test_flush_path_waits_only_in_the_empty_bucket_loop(kernel):
    import isa_stats
    ev = isa_stats.loop_waits(isa_stats.main_loop(kernel))
    g = _gather(ev)
    stores = [n for n, e in enumerate(ev) if e[1] == "store"]
    assert len(stores) == 28, len(stores)                       # the flush to a record or to a bucket: 14 x 16 bytes each
    # the flush path: from its first store to the gather, or to the loop's end where the gather comes first
    end = g[0] if g[0] > stores[0] else len(ev)
    path = ev[stores[0]:end]
    ahead = [e for e in path if e[1] == "load" and e[3] == 1]
    assert ahead, "the flush path issues no offset load of its own (outside the empty-bucket loop)"
    waits = [e for e in path if e[1] == "wait" and e[3] == 1]
    assert not waits, waits
    # the slow path is there, and it is a loop
    assert [e for e in path if e[1] == "load" and e[3] == 2]
