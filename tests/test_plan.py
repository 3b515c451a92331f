"""CPU: invariants of the MSM plan (sppark_amd/csrc/msm/msm_plan.hpp, compiled for the host by tests/emu/emu_plan.cpp)
over every size and a grid of tunables -- what the kernels' launch shapes, LDS sizes and index widths rely on -- and of
the route (msm_route.hpp): the sequence of launches the driver makes of a plan."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
MSM = os.path.join(os.path.dirname(HERE), "sppark_amd", "csrc", "msm")
KEYS = ("n", "wbits", "nwins", "NB", "nbits", "HB", "LB", "NA", "L", "chunks_per_win", "nslabs", "slab_sz", "F", "K", "K1", "G", "wpg", "big", "IB", "SH", "NG")


@pytest.fixture(scope="module")
def plan_lib():
    so, src = os.path.join(EMU, "libemu_plan.so"), os.path.join(EMU, "emu_plan.cpp")
    hdrs = [os.path.join(MSM, h) for h in ("msm_plan.hpp", "msm_route.hpp", "msm_thresholds.hpp")]
    if not os.path.exists(so) or os.stat(so).st_mtime < max(os.stat(f).st_mtime for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    up = ctypes.POINTER(ctypes.c_uint)
    L.emu_make_plan_tuned.argtypes = [ctypes.c_size_t, ctypes.c_uint, up, ctypes.c_size_t, up]
    L.emu_decode_tail_code.argtypes = [ctypes.c_uint, up]
    L.emu_make_route.argtypes = [up, up, up, up, ctypes.c_uint, up, up, ctypes.c_uint]
    L.emu_make_route.restype = ctypes.c_uint
    L.emu_make_plan.argtypes = [ctypes.c_size_t] + [ctypes.c_uint] * 10 + [ctypes.POINTER(ctypes.c_uint)]
    L.emu_make_fixed_plan.argtypes = [ctypes.c_size_t] + [ctypes.c_uint] * 3 + [ctypes.POINTER(ctypes.c_uint)]
    L.emu_make_plan_resident.argtypes = [ctypes.c_size_t, ctypes.c_uint, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint)]
    return L


def _plan(lib, n, bits=255, **kw):
    out = (ctypes.c_uint * 21)()
    lib.emu_make_plan(n, bits, kw.get("wbits", 0), kw.get("L", 0), kw.get("F", 0), kw.get("K", 0), kw.get("nslabs", 0),
                    kw.get("LB", 0), kw.get("groups", 0), kw.get("K1", 0), kw.get("records", 0), out)
    return dict(zip(KEYS, out))


def _check(p, n, bits):
    assert p["n"] == n and p["nbits"] == bits
    assert 2 <= p["wbits"] <= 24
    assert (p["nwins"] - 1) * p["wbits"] < bits <= p["nwins"] * p["wbits"]          # even split: the longest window
    assert p["nwins"] <= 128                                                          # msm_t::MAX_WINS
    assert p["NB"] == 1 << (p["wbits"] - 1)
    assert p["HB"] + p["LB"] == p["wbits"] - 1 and p["NA"] == 1 << p["HB"]
    assert p["LB"] <= 13 and p["HB"] <= 15                                            # LDS counters of level B / of the level-A histogram
    assert p["L"] >= 1 and p["chunks_per_win"] * p["L"] >= n > (p["chunks_per_win"] - 1) * p["L"]
    assert p["nslabs"] >= 1 and p["slab_sz"] * p["nslabs"] >= n
    # 4-byte level-A records (msm_sort_records.hpp): sign | index mod 2^IB | k_lo fills 32 bits; an index group is a whole
    # number (2^SH) of power-of-two slabs; every index is below NG groups; level B keeps at most 128 boundaries; no empty slab
    if p["IB"]:
        assert p["IB"] + p["LB"] == 31 and p["slab_sz"] & (p["slab_sz"] - 1) == 0 and p["slab_sz"] << p["SH"] == 1 << p["IB"]
        assert p["NG"] == ((p["nslabs"] - 1) >> p["SH"]) + 1 and 1 <= p["NG"] <= 128 and n <= p["NG"] << p["IB"]
        assert (p["nslabs"] - 1) * p["slab_sz"] < n and p["nslabs"] <= 129
    else:
        assert p["SH"] == 0 and p["NG"] == 1
    assert p["F"] >= 4                                                                # (< 3 would never shrink the record list)
    for k in ("K", "K1"):
        assert p[k] >= 1 and p[k] & (p[k] - 1) == 0 and p[k] <= p["NB"] and p["NB"] % p[k] == 0
    assert 1 <= p["G"] <= p["nwins"] and p["wpg"] * p["G"] >= p["nwins"] > p["wpg"] * (p["G"] - 1)


def test_automatic_plans_over_every_size(plan_lib):
    for bits in (255, 254, 253):
        for lg in range(0, 32):
            for n in {1 << lg, (1 << lg) + 1, (1 << lg) * 3 // 2 + 7, max(1, (1 << lg) - 1)}:
                if n > 1 << 31:
                    continue
                p = _plan(plan_lib, n, bits)
                _check(p, n, bits)
                # the automatic split: level A fits the LDS-staged scatter (2^12 partitions), partitions of ~2^14 entries
                assert p["NA"] <= 4096, (n, p)
                if (1 << 15) <= n <= (1 << 26):                                       # (above 2^26 points the 2^12 partitions outgrow
                    assert n // p["NA"] <= 18432, (n, p)                              # level B's register form: its two-pass form sorts them)


def test_run_length_fits_whole_rounds_of_resident_waves(plan_lib):
    """With the device's resident k_accumulate lanes R known (the driver's occupancy query: 131072 for the 14-limb fields,
    196608 for the 10-limb ones), the automatic run length makes windows x ceil(n / L) lanes fit k rounds of R exactly:
    never more rounds x run length than the power-of-two choice, every invariant intact, and the cases that prompted it."""
    for R in (65536, 131072, 196608):
        for bits in (255, 254):
            for lg in range(12, 29):
                for n in {1 << lg, (1 << lg) + 1, (1 << lg) * 3 // 2 + 7, (1 << lg) - 1, (1 << lg) * 5 // 4}:
                    out = (ctypes.c_uint * 21)()
                    plan_lib.emu_make_plan_resident(n, bits, R, out)
                    p = dict(zip(KEYS, out))
                    _check(p, n, bits)
                    q = _plan(plan_lib, n, bits)                                      # without the fit: the power-of-two run length
                    assert (p["wbits"], p["nwins"], p["NA"], p["K"], p["K1"]) == (q["wbits"], q["nwins"], q["NA"], q["K"], q["K1"])
                    groups = lambda pl: pl["nwins"] * -(-pl["chunks_per_win"] // 256)  # the launch: ceil(chunks / 256) groups of 256 lanes per window
                    rounds = lambda pl: -(-groups(pl) // (R // 256))
                    assert rounds(p) * p["L"] <= rounds(q) * q["L"], (n, R, p, q)
                    assert 4 <= p["L"] <= 1024
                    if p["L"] != q["L"]:
                        assert 2 <= rounds(q) <= 64 and rounds(p) * p["L"] * 100 <= rounds(q) * q["L"] * 92, (n, R, p, q)
                        assert groups(p) <= rounds(p) * (R // 256), (n, R, p)
                        if p["L"] > 4:                                                # ... tightly: one entry less per run would not fit
                            assert p["nwins"] * -(-(-(-n // (p["L"] - 1))) // 256) > rounds(p) * (R // 256), (n, R, p)
    out = (ctypes.c_uint * 21)()
    for n, L in ((1 << 17, 20), (1 << 18, 35), (300000, 40), (1 << 22, 128), (12000000, 129), (1 << 13, 8), (1 << 16, 16), (1 << 19, 64), (1 << 20, 128), (1 << 21, 128), (1 << 26, 256)):
        plan_lib.emu_make_plan_resident(n, 255, 131072, out)
        assert dict(zip(KEYS, out))["L"] == L, (n, dict(zip(KEYS, out)))


def test_tuned_plans(plan_lib):
    for n in (1, 300, 5000, 1 << 16, (1 << 20) + 3, 1 << 26):
        for wbits in (0, 2, 7, 13, 19, 24):
            for L in (0, 4, 64, 256):
                for K, K1 in ((0, 0), (2, 4), (8, 16), (4, 1 << 20)):
                    for LB in (0, 1, 9, 13):
                        for groups in (0, 1, 3, 200):
                            for records in (0, 1, 2):
                                _check(_plan(plan_lib, n, 255, wbits=wbits, L=L, K=K, K1=K1, LB=LB, groups=groups, F=3, nslabs=5,
                                             records=records), n, 255)


def test_records_tunable(plan_lib):
    """msm_tunables::records (sppark_msm_tune_records): 0 = 4-byte level-A records unless a slab count is given, 1 = 8-byte
    records always, 2 = 4-byte records also with a given slab count, the slabs then the power of two at or below n / nslabs.
    Everything else in the plan follows the size alone."""
    same = ("wbits", "nwins", "HB", "LB", "L", "F", "K", "K1", "G")
    packed = 0
    for bits in (255, 254):
        for lg in range(0, 31):
            for n in {1 << lg, (1 << lg) + 1, (1 << lg) * 3 // 2 + 7, max(1, (1 << lg) - 1)}:
                for LB in (0, 13):
                    for nslabs in (0, 1, 5, 64, 300):
                        p0, p1, p2 = (_plan(plan_lib, n, bits, LB=LB, nslabs=nslabs, records=r) for r in (0, 1, 2))
                        for p in (p0, p1, p2):
                            _check(p, n, bits)
                            assert all(p[k] == p0[k] for k in same), (n, LB, nslabs, p, p0)
                        assert p1["IB"] == 0 and p1["nslabs"] == (nslabs or min(64, max(n // 131072, min(8, max(1, n // 2048)))))
                        assert p1["slab_sz"] == -(-n // p1["nslabs"])
                        if nslabs == 0:
                            assert p2 == p0
                            continue
                        assert p0["IB"] == 0 and p0["nslabs"] == nslabs
                        # records = 2: power-of-two slabs of 2^floor(lg ceil(n / nslabs)) points (at most 2^IB), 4-byte
                        # records wherever the bounds of level B (128 index groups) and of the slab scan (129 slabs) allow
                        ib = 31 - p2["LB"]
                        lgs = min((-(-n // nslabs)).bit_length() - 1, ib)
                        ns = -(-n // (1 << lgs))
                        ng = ((ns - 1) >> (ib - lgs)) + 1
                        if ng <= 128 and ns <= 129:
                            assert (p2["IB"], p2["slab_sz"], p2["nslabs"], p2["SH"], p2["NG"]) == (ib, 1 << lgs, ns, ib - lgs, ng), (n, nslabs, p2)
                            packed += 1
                        else:
                            assert p2 == p0, (n, nslabs, p2)
    assert packed > 1000


def test_fixed_base_plans(plan_lib):
    """the one-window plan over W * n (digit, multiple) entries (msm_driver.hpp invoke_fixed)"""
    STAGE = 18 * 1024
    for bits in (255, 254):
        for lgn in range(0, 28):
            for c in range(8, 27):
                W = -(-bits // c)
                cc = -(-bits // W)                                   # the even split the driver stores
                n = (1 << lgn) + (lgn % 3)
                if W * n >= 1 << 31:
                    continue
                out = (ctypes.c_uint * 21)()
                plan_lib.emu_make_fixed_plan(n, cc, W, STAGE, out)
                p = dict(zip(KEYS, out))
                assert p["n"] == W * n and p["nwins"] == 1 and p["wbits"] == cc and p["NB"] == 1 << (cc - 1)
                assert p["HB"] + p["LB"] == cc - 1 and p["LB"] <= 13 and p["NA"] == 1 << p["HB"]
                assert p["NA"] <= 4096 or cc - 1 - 13 > 12, (n, c, p)      # staged level A unless the window leaves no choice
                assert p["chunks_per_win"] * p["L"] >= p["n"] and p["slab_sz"] * p["nslabs"] >= p["n"]
                assert p["big"] == STAGE and p["G"] == 1 and p["K1"] <= p["NB"] and p["K"] <= p["NB"]


# ---- the route: what runs after the sort (msm_route.hpp) ---------------------------------------------------------------
def _enum(name):
    """the enumerators of |name| in msm_route.hpp, in order"""
    body = re.search(r"enum %s[^{]*\{(.*?)\};" % name, open(os.path.join(MSM, "msm_route.hpp")).read(), re.S).group(1)
    return re.findall(r"\b(M[KBF]_[A-Z0-9_]+)", re.sub(r"//[^\n]*", "", body))


KERNELS, BUFS, FLAGS = _enum("msm_kernel")[:-1], _enum("msm_buf"), _enum("msm_flag")
TUN = ("wbits", "L", "F", "K", "nslabs", "LB", "groups", "K1", "records", "top", "code", "g2_path", "long_runs")
HEAD = ("nsteps", "overflow", "front", "pieces", "piece_cmax", "piece_pending", "small_sums", "flag_with_sums", "finalized", "result", "cap")
STEP = ("kernel", "flag", "rd0", "rd1", "wr0", "wr1", "block", "gx", "gy", "lds", "count", "nthreads", "fan", "t", "last", "lgGB", "lgG",
        "m", "sb", "sp")
FR = {255: 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,                 # BLS12-381
      254: 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001,                 # alt_bn128
      253: 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001}                 # BLS12-377
# the three kinds of coordinate field: (own_records, g1_loose, pairs_built, pairs_default, words, bucket_bytes, coord_bytes)
FIELD_G1 = (1, 1, 0, 0, 14, 4 * 14 * 4, 48)         # G1 over a loosely-reduced base field (14 limbs of 28 bits)
FIELD_G2 = (1, 0, 1, 1, 28, 4 * 28 * 4, 96)         # G2: Fp2 over it
FIELD_WIRE = (0, 0, 0, 0, 12, 4 * 12 * 4, 48)       # a field kept in the wire form: no records of its own


def _uints(v):
    return (ctypes.c_uint * len(v))(*v)


def plan_tuned(lib, n, bits, resident=0, **tun):
    out = (ctypes.c_uint * 21)()
    ok = lib.emu_make_plan_tuned(n, bits, _uints([tun.get(k, 0) for k in TUN]), resident, out)
    return dict(zip(KEYS, out)) if ok else None


def route(lib, plan, field, bits=255, fb_n=0, redo=0, may_defer=0, convert=0, flagged=0, stride=0, aligned16=1, top_cut=0, **tun):
    """(head, steps) of make_route, kernels / buffers / flags by name"""
    mod = [(FR[bits] >> (32 * k)) & 0xffffffff for k in range(8)]
    out = (ctypes.c_uint * 4096)()
    nw = lib.emu_make_route(_uints([plan[k] for k in KEYS]), _uints([tun.get(k, 0) for k in TUN]), _uints(field), _uints(mod), 8,
                            _uints([fb_n, redo, may_defer, convert, flagged, stride, aligned16, top_cut]), out, 4096)
    assert nw, (plan, tun)
    head = dict(zip(HEAD, out[:11]))
    head["result"] = BUFS[head["result"]]
    steps = []
    for i in range(head["nsteps"]):
        d = dict(zip(STEP, out[11 + 20 * i:31 + 20 * i]))
        d["kernel"] = KERNELS[d["kernel"]]; d["flag"] = FLAGS[d["flag"]]
        for k in ("rd0", "rd1", "wr0", "wr1"):
            d[k] = BUFS[d[k]]
        steps.append(d)
    return head, steps


BLOCK = {"MK_ACCUMULATE_G2C": 128, "MK_BUCKET_LEVEL1_PIPE": 128, "MK_BUCKET_LEVELN_PIPE": 192, "MK_BUCKET_TOP_SUM": 32, "MK_FINALIZE": 64}
G1_ONLY = {k for k in KERNELS if k.endswith(("_COOP", "_PIPE", "_LAT")) or "STAGED" in k}


def check_route(p, field, head, steps, why):
    own, g1, pairs = field[0], field[1], field[2]
    assert not head["overflow"] and head["nsteps"] < head["cap"], why
    names = [s["kernel"] for s in steps]
    for s in steps:
        assert 1 <= s["gx"] < 1 << 31 and 1 <= s["gy"] <= 65535, (why, s)
        assert s["block"] == BLOCK.get(s["kernel"], 256), (why, s)                 # what the kernel is written for
        assert s["lds"] <= 160 * 1024, (why, s)
        assert not ({s["rd0"], s["rd1"]} & {s["wr0"], s["wr1"]}) - {"MB_NONE"}, (why, s)
        assert g1 or s["kernel"] not in G1_ONLY, (why, s)
        assert pairs or s["kernel"] != "MK_ACCUMULATE_G2C", (why, s)
    wrote_image = any("MB_SUMS" in (s["wr0"], s["wr1"]) for s in steps if s["kernel"] != "MK_FINALIZE")
    assert head["finalized"] == wrote_image and (names.count("MK_FINALIZE") == 1) == bool(own and not wrote_image), (why, names)
    assert "MK_FINALIZE" not in names[:-1], (why, names)
    assert head["small_sums"] or not head["flag_with_sums"], why
    assert head["small_sums"] == ("MK_BUCKET_SMALL_BITS_COOP" in names), (why, names)
    assert head["piece_pending"] == bool(head["pieces"]), why
    # the record tree ends in a single-item level or a one-launch tail -- or the piece tree took its place
    tree = [s for s in steps if s["kernel"].startswith("MK_REDUCE")]
    if head["piece_pending"]:
        assert not tree and "MK_JOIN_RUNS" not in names, (why, names)
        pieces = steps[head["front"]:head["front"] + head["pieces"]]
        assert all(s["kernel"].startswith("MK_PIECE") for s in pieces) and [s["t"] for s in pieces] == list(range(len(pieces))), (why, names)
        assert pieces[-1]["kernel"] == "MK_PIECE_TAIL_COOP" or (pieces[-1]["last"] and 2 << pieces[-1]["t"] == head["piece_cmax"]), (why, pieces[-1])
    else:
        assert tree[-1]["kernel"].startswith("MK_REDUCE_TAIL") or (tree[-1]["last"] and tree[-1]["nthreads"] == 1), (why, tree[-1])
        nrec = 2 * p["nwins"] * p["chunks_per_win"]
        # (the kernels take the record count as 32 bits: a FORCED plan of 128 windows and runs of 4 at 2^26 points does not fit,
        # and the driver has never refused it -- the automatic plans stay far below)
        assert all(not s["last"] for s in tree[:-1]) and (tree[0]["count"] == nrec or (nrec >= 1 << 32 and p["L"] <= 4)), (why, names)
        for a, b in zip(tree, tree[1:]):
            assert b["count"] == 2 * a["nthreads"] and (b["rd0"], b["rd1"]) == (a["wr0"], a["wr1"]), (why, a, b)
    # the bucket sums: the chunk factors multiply to the bucket count; the result is what the last summing step wrote
    sums = [s for s in steps if s["kernel"].startswith("MK_BUCKET")]
    if head["small_sums"]:
        assert [s["kernel"] for s in sums] == ["MK_BUCKET_SMALL_BITS_COOP", "MK_BUCKET_TOP_SUM_COOP"] and p["NB"] <= 256, (why, names)
        assert head["result"] == sums[-1]["wr0"], why
    else:
        prod = 1
        for s in sums:
            if "LEVEL" in s["kernel"]:
                prod *= s["fan"]
            elif "TOP_BITS" in s["kernel"]:
                prod *= s["count"]
                assert s["count"] == 1 << s["m"] and 32 <= s["count"], (why, s)
        assert prod == p["NB"] and sums[0]["kernel"].startswith("MK_BUCKET_LEVEL1"), (why, names)
        last = sums[-1]
        assert head["result"] == (last["wr0"] if "TOP_SUM" in last["kernel"] else last["wr1"]), (why, last)
    if own and not head["finalized"]:
        assert steps[-1]["rd0"] == head["result"], why


CODES = tuple(range(0, 12)) + (26, 46, 79)


def test_routes_over_every_size(plan_lib):
    """every size with its neighbours x the three field kinds x every switch code x first pass (alone: the caller reads the
    piece tree's flag; one of several chunks: nobody does) / second pass, one or several window groups"""
    seen = set()
    for bits in (255, 254, 253):
        for lg in range(0, 32):
            for n in sorted({1 << lg, (1 << lg) + 1, (1 << lg) * 3 // 2 + 7, max(1, (1 << lg) - 1)}):
                if n > 1 << 31:
                    continue
                for field in (FIELD_G1, FIELD_G2, FIELD_WIRE):
                    for code in CODES:
                        for groups in (0, 3):
                            tun = dict(code=code, groups=groups, long_runs=int(field is FIELD_G2), g2_path=code % 3 if field is FIELD_G2 else 0)
                            p = plan_tuned(plan_lib, n, bits, 131072, **tun)
                            _check(p, n, bits)
                            for redo, may_defer in ((0, 1), (0, 0), (1, 0)):
                                why = (bits, n, field, tun, redo, may_defer)
                                head, steps = route(plan_lib, p, field, bits, redo=redo, may_defer=may_defer, convert=field[0], flagged=n & 1,
                                                    stride=2 * field[6] + 8 * (n & 1), aligned16=lg & 1, **tun)
                                check_route(p, field, head, steps, why)
                                assert head["front"] == (0 if redo else 1 + field[0]) and (redo or may_defer or not head["pieces"]), why
                                assert not (redo and head["pieces"]) and not (p["G"] > 1 and (head["pieces"] or head["small_sums"])), why
                                seen.update(s["kernel"] for s in steps)
    assert seen == set(KERNELS), set(KERNELS) - seen                # every kernel is reached by some size and switch


def test_routes_of_tuned_and_fixed_base_plans(plan_lib):
    """the tunables grid of test_tuned_plans with the bucket sums' own knobs (top, K1), and the one-window fixed-base plans"""
    for n in (1, 300, 5000, 1 << 16, (1 << 20) + 3, 1 << 26):
        for wbits in (0, 2, 7, 13, 19, 24):
            for L in (0, 4, 64, 256):
                for K, K1 in ((0, 0), (2, 4), (8, 16), (4, 1 << 20)):
                    for groups in (0, 1, 3, 200):
                        for top, code, field in ((0, 0, FIELD_G1), (1, 4, FIELD_G1), (64, 0, FIELD_G1), (0, 0, FIELD_G2), (256, 0, FIELD_WIRE)):
                            tun = dict(wbits=wbits, L=L, K=K, K1=K1, groups=groups, F=3, nslabs=5, top=top, code=code)
                            p = plan_tuned(plan_lib, n, 255, **tun)
                            head, steps = route(plan_lib, p, field, may_defer=1, convert=field[0], stride=2 * field[6], **tun)
                            check_route(p, field, head, steps, (n, tun, field))
    out = (ctypes.c_uint * 21)()
    for lgn in range(0, 28):
        for c in range(8, 27):
            W = -(-255 // c)
            n = (1 << lgn) + (lgn % 3)
            if W * n >= 1 << 31:
                continue
            plan_lib.emu_make_fixed_plan(n, -(-255 // W), W, 18 * 1024, out)
            p = dict(zip(KEYS, out))
            head, steps = route(plan_lib, p, FIELD_G1, fb_n=n, may_defer=0)
            check_route(p, FIELD_G1, head, steps, (n, c))
            assert not head["pieces"] and not head["small_sums"] and head["front"] == 1, (n, c)
