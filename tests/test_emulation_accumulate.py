"""CPU: accumulate_chunk (msm/msm_kernels.hpp) on the host against a straightforward per-bucket sum, on grouped lists
built to hit the paths of the walk that keeps its bucket offsets one boundary ahead (next = o[b+1], next2 = o[b+2]) and
its point gather one entry ahead, undecoded (tests/emu/emu_accumulate.cpp: bit-for-bit images of every record and
bucket, fill patterns where nothing may be written, and the offsets, the list and the point records each end at an
inaccessible page, so a read past o[NB] or past the last entry is a fault here, not a pass).

The lists, per case (bucket sizes in list order; L = entries per work item):
  * a boundary followed by one and by many empty buckets (the slow path of the offsets kept ahead);
  * a boundary AT the last entry of a work item's run, and one entry before it;
  * the window's last bucket NB - 1 in use (there is no o[NB + 1]), and a window that ends in empty buckets;
  * runs of one and two entries, several in a row (a boundary in consecutive iterations);
  * a list that is no multiple of L, a single entry, an empty window;
  * the point at infinity as the first entry of a run, in the middle, and as the entry that is prefetched last (the last
    of a work item's run, and the last of the list);
  * negated entries throughout.
G1 over BLS12-381 and alt_bn128 (the prefetching walk) and G2 over alt_bn128 (the walk without prefetch)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import recipe

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _emu(feature, g2=False):
    so = os.path.join(EMU, "libemu_accumulate_%s%s.so" % (feature, "_G2" if g2 else ""))
    src = os.path.join(EMU, "emu_accumulate.cpp")
    csrc = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc")
    newest = max(os.stat(os.path.join(r, f)).st_mtime for r, _, fs in os.walk(csrc) for f in fs)
    newest = max(newest, os.stat(src).st_mtime)
    if not os.path.exists(so) or os.stat(so).st_mtime < newest:
        if not os.path.exists(HIPCC):
            pytest.skip("hipcc not available")
        subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared",
                               "-DFEATURE_" + feature] + (["-DSPPARK_G2"] if g2 else []) + ["-o", so, src])
    L = ctypes.CDLL(so)
    vp, sz, ci, cu = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint
    L.emu_accumulate_check.argtypes = [vp, sz, sz, ci, vp, vp, cu, cu, vp]
    return L


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


NPTS = 48
INF = (0, 5, 17)                                                # the points at infinity of the point set


def _lists():
    """(name, bucket sizes, L, {list position: point index}) -- positions not named take points in a fixed shuffle"""
    E = []
    E.append(("one empty bucket behind a boundary", [3, 0, 4, 2, 0, 3], 6, {}))
    E.append(("many empty buckets behind a boundary", [2, 0, 0, 0, 0, 0, 0, 5, 0, 0, 3, 0], 5, {}))
    E.append(("boundary at the last entry of a run", [3, 4, 1, 5, 3], 8, {}))                    # bucket 2 is entry 7 = the last of chunk 0
    E.append(("boundary one before the last entry of a run", [3, 3, 2, 5, 3], 8, {}))
    E.append(("bucket ends with the run", [4, 4, 8, 3, 5], 8, {}))
    E.append(("last bucket in use", [0, 2, 0, 3, 1, 6], 4, {}))
    E.append(("only the last bucket", [0, 0, 0, 0, 0, 0, 0, 9], 4, {}))
    E.append(("window ends in empty buckets", [5, 1, 2, 0, 0, 0], 3, {}))
    E.append(("runs of one", [1] * 13, 5, {}))
    E.append(("runs of one and two", [1, 2, 1, 1, 2, 2, 1, 0, 1, 2], 4, {}))
    E.append(("runs of one between empty buckets", [1, 0, 1, 0, 0, 1, 1, 0, 2, 0], 16, {}))
    E.append(("one bucket over many runs", [0, 37, 0, 2], 4, {}))
    E.append(("not a multiple of L", [6, 5, 7, 1], 8, {}))
    E.append(("a single entry", [0, 1, 0], 8, {}))
    E.append(("an empty window", [0, 0, 0, 0], 8, {}))
    E.append(("L = 1", [2, 0, 3, 1], 1, {}))
    E.append(("L = 2", [2, 0, 3, 1, 1, 4], 2, {}))
    # infinity: first of a run (positions 0 and 8), in the middle (3, 10), prefetched last (7 = last of chunk 0; 18 = last of the list)
    E.append(("infinity first / middle / last of a run", [3, 2, 6, 1, 7], 8, {0: INF[0], 3: INF[1], 7: INF[2], 8: INF[0], 10: INF[1], 18: INF[2]}))
    E.append(("infinity at bucket boundaries", [2, 1, 1, 3, 2, 0, 4], 5, {1: INF[0], 2: INF[1], 3: INF[2], 4: INF[0], 9: INF[1], 12: INF[2]}))
    E.append(("a bucket of infinities", [2, 3, 2], 4, {2: INF[0], 3: INF[1], 4: INF[2]}))
    rng = np.random.default_rng(2608)
    for k in range(12):                                         # random windows: ~40 % empty buckets, runs of 1 .. 9
        NB = int(rng.integers(2, 40))
        sizes = [int(rng.integers(1, 10)) if rng.random() > 0.4 else 0 for _ in range(NB)]
        total = sum(sizes)
        where = {int(p): INF[int(rng.integers(0, 3))] for p in rng.integers(0, max(total, 1), 4)} if total else {}
        E.append(("random %d" % k, sizes, int(rng.integers(1, 20)), where))
    return E


@pytest.mark.parametrize("curve,feature,g2", [(0, "BLS12_381", False), (1, "BN254", False), (3, "BN254", True)])
@pytest.mark.parametrize("flagged", [False, True])
def test_accumulate_chunk_against_per_bucket_sums(oracle, curve, feature, g2, flagged):
    L = _emu(feature, g2)
    pts, _sc = recipe.msm_inputs(curve, NPTS, 808 + curve, ndistinct=NPTS, edge=False, flagged=flagged)
    pts = pts.copy()
    for i in INF:                                               # infinity: all-zero coordinates (and the flag byte of the flagged format)
        pts[i] = 0
        if flagged:
            pts[i, pts.shape[1] - 8] = 1                        # (X | Y | flag byte + padding)
    rng = np.random.default_rng(99 + curve)
    seen_direct = 0
    for name, sizes, LL, where in _lists():
        total = sum(sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        finite = np.array([i for i in range(NPTS) if i not in INF])
        idx = finite[rng.integers(0, len(finite), total)].astype(np.uint32) if total else np.zeros(0, dtype=np.uint32)
        for pos, pi in where.items():
            idx[pos] = pi
        neg = (rng.random(total) < 0.5).astype(np.uint32)
        sorted_ = (idx | (neg << 31)).astype(np.uint32)
        info = np.zeros(3, dtype=np.uint32)
        bad = L.emu_accumulate_check(P(pts), pts.shape[1], NPTS, int(flagged), P(sorted_), P(off), len(sizes), LL, P(info))
        assert bad == 0, (name, sizes, LL, bad)
        assert int(info[2]) == (total + LL - 1) // LL + 1, name
        seen_direct += int(info[1])
    assert seen_direct > 50                                     # buckets that were flushed straight from the walk
