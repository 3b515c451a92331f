"""GPU: the automatic MSM plans against the oracle at every size regime they take.

The plan (csrc/msm/msm_plan.hpp) changes shape at many sizes between the few the other tests pin: the window width, the
sort split (by the CEILING of lg n, so 2^k and 2^k + 1 differ), 4-byte records and their index groups, the first
bucket-sum chunk, the run length the device's resident lanes decide (non-powers of two such as 39 or 86), the piece tree.
Here the sizes come from the plan itself: every size of a dense grid is reduced to a signature of what the kernels see,
and the smallest size of every signature runs against the oracle through the period fold (oracle/fold.py) with points of
an odd prime period, so that an index slip of k 2^m reads a different point.  `pytest -s` prints the signature -> size
tables.  G2 likewise over its run-length regimes (the long runs of the wave-pair accumulation over the 14-limb fields)."""
import numpy as np
import pytest

import recipe

pytestmark = pytest.mark.gpu
CURVES = [(0, "bls12_381"), (1, "bn254"), (4, "bls12_377"), (6, "pallas"), (7, "vesta")]
G2 = [("bls12_381", 2), ("bn254", 3), ("bls12_377", 5)]
PER = 2039                                  # odd prime: k 2^m = 0 mod 2039 only for k = 0 mod 2039
PER_G2 = 509
SIG = ("window_bits", "low_bits", "partitions", "bucket_chunk", "first_bucket_chunk", "fan_in", "packed_records",
       "index_groups>1", "window_groups", "run_length_pow2", "piece_tree")


def _ladder():
    """n = 2^k (1 + j/8), 2^k + 1 and 2^(k+1) - 1 for k = 15 ... 25"""
    ns = set()
    for k in range(15, 26):
        ns.update((1 << k) * (8 + j) // 8 for j in range(8))
        ns.update(((1 << k) + 1, (1 << (k + 1)) - 1))
    return sorted(ns)


def _signature(p):
    L = p["run_length"]
    return (p["window_bits"], p["low_bits"], p["partitions"], p["bucket_chunk"], p["first_bucket_chunk"], p["fan_in"],
            p["packed_records"], p["index_groups"] > 1, p["window_groups"], L & (L - 1) == 0, p["piece_tree_max"] > 0)


def _signatures(ctx):
    """{signature: smallest ladder size with it} of the context's automatic plan, printed as a table"""
    first = {}
    for n in _ladder():
        first.setdefault(_signature(ctx.plan(n)), n)
    print("\n%s: %d plan signatures over %d sizes" % (ctx.curve, len(first), len(_ladder())))
    print("  %10s  %s" % ("n", "  ".join(SIG)))
    for sig, n in sorted(first.items(), key=lambda t: t[1]):
        print("  %10d  %s  (run_length %d)" % (n, sig, ctx.plan(n)["run_length"]))
    return first


def _skew(sc, n):
    """all scalars equal (every window one level-A partition) and every second one zero (half-empty record lists)"""
    eq = sc[:n].clone(); eq[:] = sc[PER + 1]
    half = sc[:n].clone(); half[::2] = 0
    return (("all equal", eq), ("every second zero", half))


@pytest.mark.parametrize("curve,name", CURVES)
def test_msm_plan_ladder_vs_oracle(oracle, libs, curve, name):
    """The smallest size of every automatic plan signature from 2^15 to 2^26 - 1 points: uniform scalars (the first period
    carries the recipe's edge rows: 0, r - 1, (r +- 1) / 2, 1, a doubling, P and -P; point 3 is infinity) against the
    oracle on the folded scalars.  BLS12-381 and alt_bn128 (the two limb layouts of the bucket field): also all-equal and
    every-second-zero scalars at the smallest size of every window width."""
    import torch
    import sppark_amd
    from sppark_amd import synth
    from oracle import fold
    O = oracle
    r = O.FR_MODULUS[curve]
    ctx = sppark_amd.MsmContext(name, stream=torch.cuda.current_stream().cuda_stream)
    first = _signatures(ctx)
    top = max(first.values())
    base, sc0 = recipe.msm_inputs(curve, PER, 0x1adde7 + curve, ndistinct=PER, edge=True)
    d_base = torch.from_numpy(base).cuda()
    pts = d_base[torch.arange(top, device="cuda") % PER].contiguous()
    sc = synth.uniform_scalars(top, name, seed=1500 + curve)
    sc[:PER] = torch.from_numpy(sc0).cuda()
    widths = set()
    for sig, n in sorted(first.items(), key=lambda t: t[1]):
        cases = [("uniform", sc[:n])]
        if name in ("bls12_381", "bn254") and sig[0] not in widths:
            widths.add(sig[0])
            cases += _skew(sc, n)
        for what, s_ in cases:
            got = sppark_amd.to_affine(ctx.invoke(pts[:n], s_), name)
            exp = O.msm_affine(curve, base, fold.fold_scalars(s_, PER, r), algo=0, param=8)
            assert (got == exp).all(), (name, n, sig, what)
    ctx.close()


@pytest.mark.parametrize("curve,name", [(0, "bls12_381"), (1, "bn254")])
def test_msm_host_inputs_ragged_last_chunk_vs_oracle(oracle, libs, curve, name):
    """Host-resident inputs of 2^21 + 3 * 2039 + 5 points go through the chunked path in 2^20-point chunks, the last one
    6122 points (a plan of its own), per limb layout of the bucket field, against the oracle."""
    import torch
    import sppark_amd
    from sppark_amd import synth
    from oracle import fold
    O = oracle
    n = (1 << 21) + 3 * PER + 5
    base, _ = recipe.msm_inputs(curve, PER, 0x4057 + curve, ndistinct=PER, edge=True)
    pts = base[np.arange(n) % PER]
    sc = synth.uniform_scalars(n, name, seed=2100 + curve).cpu().numpy()
    ctx = sppark_amd.MsmContext(name)
    got = sppark_amd.to_affine(ctx.invoke(pts, sc), name)
    assert ctx.last_chunks() == 3 and n % (1 << 20) == 3 * PER + 5
    assert (got == O.msm_affine(curve, base, fold.fold_scalars(sc, PER, O.FR_MODULUS[curve]), algo=0, param=8)).all()
    ctx.close()


def test_msm_records_tunable_vs_oracle(oracle, libs):
    """sppark_msm_tune_records at a size that packs by default (2^23 + 2039 points): 0 = 4-byte records unless a slab count
    is given, 1 = 8-byte records, 2 = 4-byte records with the given slab count rounded to power-of-two slabs (here five
    asked for: nine slabs of 2^20 in two index groups) -- the plan follows the knob and every setting equals the oracle."""
    import torch
    import sppark_amd
    from sppark_amd import synth
    from oracle import fold
    O = oracle
    n = (1 << 23) + PER
    base, _ = recipe.msm_inputs(O.BLS12_381, PER, 0x7ec0, ndistinct=PER, edge=True)
    pts = torch.from_numpy(base).cuda()[torch.arange(n, device="cuda") % PER].contiguous()
    sc = synth.uniform_scalars(n, "bls12_381", seed=2300)
    exp = O.msm_affine(O.BLS12_381, base, fold.fold_scalars(sc, PER, O.FR_MODULUS[O.BLS12_381]), algo=0, param=8)
    ctx = sppark_amd.MsmContext("bls12_381", stream=torch.cuda.current_stream().cuda_stream)
    for records, nslabs, packed in ((0, 0, True), (1, 0, False), (2, 0, True), (0, 5, False), (1, 5, False), (2, 5, True)):
        ctx.tune_records(records); ctx.tune(nslabs=nslabs)
        p = ctx.plan(n)
        assert p["packed_records"] == packed, (records, nslabs, p)
        if nslabs and packed:
            lgs = (-(-n // nslabs)).bit_length() - 1
            assert p["slab_points"] == 1 << lgs and p["slabs"] == -(-n // (1 << lgs)) and p["index_groups"] == 2, p
        elif nslabs:
            assert p["slabs"] == nslabs, p
        got = sppark_amd.to_affine(ctx.invoke(pts, sc))
        assert (got == exp).all(), (records, nslabs)
    ctx.close()


@pytest.mark.parametrize("name,curve", G2)
def test_msm_g2_plan_ladder_vs_oracle(oracle, libs, name, curve):
    """G2 at 2^15 ... 2^24 points, 2^16 + 1 and 2^20 - 1, under both accumulation kernels (sppark_msm_g2_path 1: a wave pair
    per addition, with the long runs L = 32 / 64 / 128 over the 14-limb fields from 2^16 to 2^25 - 1 points; 2: one lane
    per addition): flagged points of period 509 (the recipe's edge rows, point 3 infinity with garbage coordinates under
    its flag), uniform scalars, against the oracle on the folded scalars.  Both sides of every run-length boundary:
    2^15 / 2^16, 2^18 / 2^19, 2^19 / 2^20, and 2^24, the last size with long runs (2^22 is the bench's shape)."""
    import torch
    import sppark_amd
    from sppark_amd import synth
    from oracle import fold
    O = oracle
    r = O.FR_MODULUS[curve]
    sizes = sorted({1 << k for k in range(15, 25)} | {(1 << 16) + 1, (1 << 20) - 1})
    base, sc0 = recipe.msm_inputs(curve, PER_G2, 0x92 + curve, ndistinct=PER_G2, flagged=True)
    d_base = torch.from_numpy(base).cuda()
    pts = d_base[torch.arange(sizes[-1], device="cuda") % PER_G2].contiguous()
    sc = synth.uniform_scalars(sizes[-1], name, seed=2400 + curve)
    sc[:PER_G2] = torch.from_numpy(sc0).cuda()
    try:
        for n in sizes:
            exp = O.msm_affine(curve, base, fold.fold_scalars(sc[:n], PER_G2, r), algo=0, param=8)
            for path in (1, 2):
                sppark_amd.set_g2_path(path, name)
                got = sppark_amd.to_affine_g2(sppark_amd.multi_scalar_mult_fp2_arkworks(pts[:n], sc[:n], name), name)
                assert (got == exp).all(), (name, n, path)
    finally:
        sppark_amd.set_g2_path(0, name)
