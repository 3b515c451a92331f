// Work-group sizes and routing thresholds of the MSM kernels that the HOST decides by (msm_route.hpp), with the measurements
// behind them.  No HIP: the kernel headers include this file for the sizes their launch bounds and LDS images use, the
// route and tests/emu include it with a plain host compiler.  The kernels themselves are described where they are defined.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
# define SPPARK_HOST_DEVICE __host__ __device__
#else
# define SPPARK_HOST_DEVICE
#endif

namespace sppark_amd {

// The nbits scalar bits are split EVENLY over the windows (msm_kernels.hpp recode_digits): the first nbits % nwins are one
// bit longer.  (Also used by the host Horner and the piece tree's sizing.)
SPPARK_HOST_DEVICE inline unsigned window_len(unsigned w, unsigned nwins, unsigned nbits)
{   return nbits / nwins + (w < nbits % nwins ? 1u : 0u);   }

// ---- the record tree (msm_kernels.hpp, msm_coop_kernels.hpp) ---------------------------------------------------------
// k_reduce_tail: from the level with <= REDUCE_TAIL_NT work items on, one work-group runs the remaining levels.
// (256 lanes = one wave per SIMD, like the other cold kernels: a 1024-lane work-group would cap the kernel at 128
// registers -- 187 spilled for the 14-limb field, 3x slower per addition -- and, over Fp2, call the outlined addition,
// which is compiled for up to 512, from a kernel that owns 128: that build hung the G2 tests)
static constexpr unsigned REDUCE_TAIL_NT = 256;
static constexpr unsigned COOP_NT = 256;        // the cooperative kernels' work-group: four waves
// From the level with <= COOP_TREE_MAX work items on -- one work-group per CU -- the cooperative addition (9 us against 16,
// profiles/r04_chain_bench.log) sets the pace of the record tree (k_reduce_runs_coop).
static constexpr unsigned COOP_TREE_MAX = 16384;

// ---- the piece tree (msm_piece_kernels.hpp, msm_coop_kernels.hpp) ----------------------------------------------------
// Every level of the piece tree from t0 on in ONE launch (k_piece_tail_coop): the levels of <= PIECE_FUSE_MAX work items are
// ~15 us each as launches of their own.  Same box, wall (profiles/r06_msm_piece_tail_ab.log): 2^10 0.426 -> 0.406 ms,
// 2^12 0.482 -> 0.463, 2^14 0.550 -> 0.541, 2^16 0.800 -> 0.788; from 2^16 work items on the lane-per-addition launches are
// faster (2^14: 0.585 with the levels of 2^16 items in here).
static constexpr size_t PIECE_FUSE_MAX = 32768;
// The narrow end of the tree in ONE launch (k_piece_tail_coop): every level from t0 on, a work-group owning 2^lgGB buckets
// with ALL their pairs, so that a level only waits for the work-group's own stores.  Work item |idx| of work-group |wg| at
// level t: bucket (wg << lgGB) + idx % 2^lgGB, pair idx >> lgGB.  lgGB fills the 64 lanes of a cooperative addition at
// level t0: 2^lgGB (cmax >> (t0 + 1)) >= 64 where the buckets allow.
static inline unsigned piece_tail_lgGB(unsigned cmax, unsigned t0)
{
    const unsigned pm = cmax >> (t0 + 1);
    unsigned lg = 0;
    while ((pm << lg) < 64) lg++;
    return lg;
}
// first level of the one-launch end: the first whose work items (buckets x pair slots) are at most |fuse_max|; the levels
// before it are launches of their own (lane-per-addition kernels: throughput, not latency)
static inline unsigned piece_tail_t0(size_t nbuckets, unsigned cmax, size_t fuse_max)
{
    unsigned t = 0;
    while ((cmax >> (t + 1)) >= 1 && nbuckets * (cmax >> (t + 1)) > fuse_max) t++;
    return t;
}
// CMAX for an average bucket of |avg_pieces| pieces: a power of two >= 3 x + 4.  (Uniform scalars are NOT uniform digits in
// the top window: it is a bit shorter than the others when the scalar bits do not divide evenly, and the modulus cuts its
// range -- BLS12-381's r = 0x73ed... leaves 115 of the 128 values of a 7-bit top window, all of magnitude <= 64: 2.2 x the
// entries per bucket.  The extra levels are launches of a few lanes that find nothing to add.)
static inline unsigned piece_cmax_exact(size_t want)            // the power of two >= want
{
    unsigned c = 2;
    while (c < want && c < 4096) c <<= 1;
    return c;
}
static inline unsigned piece_cmax(size_t avg_pieces) { return piece_cmax_exact(3 * avg_pieces + 4); }

// ---- the bucket sums (msm_kernels.hpp, msm_coop_kernels.hpp) ---------------------------------------------------------
// one wave per SIMD on 256 CUs: bucket-sum grids up to this size run the paired-product one-wave kernels.  (Larger,
// work-bound grids are faster with the two-wave kernels: forcing the one-wave ones everywhere costs the tail of a
// 2^26-point MSM 2.0 ms and 0.5 ms at 2^24, profiles/r04_msm_lat_lanes_negative.log.)
static constexpr size_t LAT_LANES = 65536;
// The chunked levels in cooperative form for grids of at most one work-group of four waves per CU (<= COOP_LEVEL_MAX work
// items: MSMs of <= 2^16 points, and the last chunked level of larger ones); also the piece tree's levels.
// (24576 or 32768 -- 1.5 or 2 rounds of work-groups -- change nothing measurable: profiles/r04_msm_coop_level_max.log)
static constexpr unsigned COOP_LEVEL_MAX = 16384;
// The subset-sum top (k_bucket_top_bits): once a window is down to M = 2^m <= BUCKET_TOP_MAX items; its work-group.
static constexpr unsigned BUCKET_TOP_MAX = 4096, BUCKET_TOP_NT = 256;
// pieces per subset sum (sb) and per plain sum (sp) for |nitems| items and work-groups of |nt| lanes.  Measured
// (profiles/r06_msm_top_cut_sweep.log, 2^18 .. 2^24 points): cutting the PLAIN sum of a 4096-item top in two -- the one
// work-group with twice the additions per lane of all the others -- is the whole gain (tail 2^19 0.79 -> 0.72 ms, 2^20
// 0.99 -> 0.94, 2^21 1.24 -> 1.16, 2^22 1.35 -> 1.30); more pieces (2 / 4, 2 / 8: twice the work-groups, two per CU) bring
// nothing further -- what is left is the tree and the doublings -- and at 2048 items (2^18 points) nothing changes.
// At most 32 parts per window (k_bucket_top_sum_coop's image).
static inline void bucket_top_cut(unsigned nitems, unsigned nt, unsigned& sb, unsigned& sp)
{
    sb = 1;
    sp = nitems >= 16 * nt ? 2 : 1;
}
// k_bucket_top_bits_coop's dynamic LDS for a field of |nl| words
// (the exchange area of the cooperative operations + an image of COOP_NT / 2 points: 56 KB on fourteen limbs, two work-groups per CU)
static inline size_t top_bits_coop_lds(size_t nl) { return 2 * 4 * nl * 64 * 4 + 4 * nl * (COOP_NT / 2) * 4; }
// the small windows' form of the same sum, straight from the buckets (k_bucket_small_bits_coop): windows of up to this many buckets
static constexpr unsigned SMALL_SUMS_MAX_NB = 256;

// ---- G2 by wave pairs (msm_g2c_kernels.hpp) --------------------------------------------------------------------------
static constexpr unsigned G2C_NT = 128;             // a pair of waves

} // namespace sppark_amd
