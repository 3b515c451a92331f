// The ROUTE of an MSM: which kernels run after the sort, with which grids, LDS sizes and buffers -- as data.
// A pure function of the plan, the tunables, a few facts about the coordinate field and the call at hand; no HIP and no
// device pointers (the scalar modulus comes as a pointer to its words).  msm_driver.hpp enqueue() launches what it says,
// step by step; tests/emu/emu_plan.cpp returns it as integers, so that "what runs at size n" is checked at every size
// without a GPU (tests/test_plan.py, tests/test_msm_route.py).
// The thresholds it decides by, and the measurements behind them, are in msm_thresholds.hpp.
#pragma once
#include "msm_plan.hpp"
#include <cmath>
#include <cstdint>

namespace sppark_amd {

// one value per kernel template (and per value of its bool parameter)
enum msm_kernel : unsigned char {
    MK_CONVERT, MK_CONVERT_FLAGGED,                 // k_convert_points<FP, false / true>
    MK_CONVERT_STAGED, MK_CONVERT_STAGED_FLAGGED,   // k_convert_points_staged<FP, false / true>
    MK_ACCUMULATE, MK_ACCUMULATE_FLAGGED,           // k_accumulate<FP, false / true>
    MK_ACCUMULATE_G2C,
    MK_PIECE_LEVEL, MK_PIECE_LEVEL_COOP, MK_PIECE_TAIL_COOP,
    MK_JOIN_RUNS, MK_REDUCE_RUNS, MK_REDUCE_RUNS_COOP, MK_REDUCE_TAIL, MK_REDUCE_TAIL_COOP,
    MK_BUCKET_SMALL_BITS_COOP,
    MK_BUCKET_LEVEL1, MK_BUCKET_LEVEL1_LAT, MK_BUCKET_LEVEL1_PIPE, MK_BUCKET_LEVEL1_COOP,      // (in the order of msm_sums_form)
    MK_BUCKET_LEVELN, MK_BUCKET_LEVELN_LAT, MK_BUCKET_LEVELN_PIPE, MK_BUCKET_LEVELN_COOP,
    MK_BUCKET_TOP_BITS, MK_BUCKET_TOP_SUM, MK_BUCKET_TOP_BITS_COOP, MK_BUCKET_TOP_SUM_COOP,
    MK_FINALIZE,
    MK_COUNT
};

// what a step reads and writes: the driver maps a role to a pointer into its scratch.  (MB_POINTS, MB_CONV and MB_SUMS are
// informational -- the kernels that take them have them as fixed arguments -- and serve the read / write checks of the tests.)
enum msm_buf : unsigned char {
    MB_NONE, MB_POINTS,                             // the MSM's points (wire form, or the field's own records)
    MB_CONV,                                        // ... converted by this MSM
    MB_BUCKETS,
    MB_KEY_A, MB_PT_A, MB_KEY_B, MB_PT_B,           // the two record lists of the tree
    MB_KEY_C,                                       // k_join_runs' filtered keys (the points stay in MB_PT_A)
    MB_A1, MB_W1, MB_A2, MB_W2,                     // the two (sum, weighted sum) sets of the bucket-sum chain
    MB_SUMS                                         // the window sums' wire image
};
enum msm_flag : unsigned char {
    MF_NONE,
    MF_SCRATCH,                                     // the flag word of the scratch blob: cleared before use
    MF_SMALL                                        // the small sizes' word: zero between MSMs, handed over and cleared by the last kernel
};

struct msm_step {
    msm_kernel kernel;
    msm_flag flag;                      // piece tree: "a bucket had more pieces than cmax"; record tree: k_join_runs' "a long segment exists"
    msm_buf rd[2], wr[2];               // records: (keys, points); bucket sums: (sums, weighted sums)
    unsigned short block;
    unsigned gx, gy, lds;               // grid in work-groups, dynamic LDS bytes
    // the scalars that differ from step to step (what does not is the plan's)
    unsigned count;                     // points / records / items per window the step reads
    unsigned nthreads;                  // record tree: work items
    unsigned fan;                       // record tree: fan-in F; bucket sums: buckets / items per work item (K1, K)
    unsigned t, last;                   // piece tree: level, "the last level"; record tree: last
    unsigned lgGB;                      // k_piece_tail_coop: log2 buckets per work-group
    unsigned lgG;                       // bucket sums: log2 buckets per item
    unsigned m, sb, sp;                 // subset-sum top: log2 items, pieces per subset sum / per plain sum
};

// what the route must know of the coordinate field (msm_t's compile-time facts)
struct msm_field {
    bool own_records;                   // its own point / bucket records: conversion, k_finalize (G1 and G2 over the loosely-reduced fields)
    bool g1_loose;                      // ... over the base field: the cooperative, two-wave and low-latency kernels exist
    bool pairs_built;                   // the wave-pair accumulation (k_accumulate_g2c) exists
    bool pairs_default;                 // ... and is the default (the 14-limb base fields)
    unsigned words;                     // 32-bit words of a coordinate in a bucket record
    unsigned bucket_bytes;              // a bucket record
    unsigned coord_bytes;               // a coordinate in the wire form
    const uint32_t* scalar_mod;         // the scalar field's modulus
    unsigned scalar_words;
};

// the call at hand
struct msm_call {
    unsigned fb_n = 0;                  // fixed-base mode: points (the plan is ONE window over fb_nwins * fb_n entries); 0 = not
    bool redo = false;                  // second pass: only the fan-in tree over the records the piece tree left, and everything after it
    bool may_defer = false;             // the caller looks at the piece tree's flag after this MSM (one chunk)
    bool convert = false;               // the points are in wire form and the field has its own records
    bool flagged = false;               // wire points with an infinity flag behind the coordinates
    size_t stride = 0;                  // bytes between wire points
    bool aligned16 = false;             // ... whose base is 16-byte aligned
    unsigned top_cut = 0;               // tuning builds: "sb sp" of the subset-sum top as two digits (0 = bucket_top_cut)
    unsigned short_bits = 0;            // short scalars (k_breakdown_short): every scalar is below 2^short_bits; 0 = full width, folded below r/2
};

struct msm_route {
    static constexpr unsigned CAP = 96; // (the longest: 2 + 10 piece levels + k_join_runs + 19 tree levels + 24 sum levels + 3)
    msm_step steps[CAP];
    unsigned nsteps = 0;
    bool overflow = false;              // more than CAP steps (a chunk factor of 1, say): the caller refuses the call
    unsigned front = 0;                 // steps before the tail: [conversion,] accumulation (one step: the driver launches it per window group)
    unsigned pieces = 0;                // ... of the piece tree, which follow
    unsigned piece_cmax = 0;
    bool piece_pending = false;         // the piece tree ran and the fan-in tree was left out
    bool small_sums = false;            // the small windows' sums
    bool flag_with_sums = false;        // the piece tree's flag travels behind the window sums (MF_SMALL)
    bool finalized = false;             // a step wrote the wire image: no k_finalize
    msm_buf result = MB_NONE;           // the window sums (bucket records)

    msm_step& add(msm_kernel k, unsigned gx, unsigned gy, unsigned block, unsigned lds = 0)
    {
        if (nsteps == CAP) { overflow = true; nsteps--; }
        msm_step& s = steps[nsteps++];
        s = msm_step();
        s.kernel = k; s.gx = gx; s.gy = gy; s.block = (unsigned short)block; s.lds = lds;
        return s;
    }
};

static inline unsigned div_up(size_t a, size_t b) { return (unsigned)((a + b - 1) / b); }

// pieces per bucket the piece tree of a small MSM takes, 0 = the record list goes through k_join_runs / the fan-in tree:
// one window group, not the fixed-base window, buckets longer than the join's walk, at most 2^10 pieces
// (|short_bits|: msm_call)
static inline unsigned piece_tree_cmax(const msm_plan& p, const msm_switches& sw, unsigned fb_n, const uint32_t* scalar_mod, unsigned scalar_words,
                                       unsigned short_bits = 0)
{
    if (p.G > 1 || fb_n || sw.no_piece_tree) return 0;
    if ((size_t)p.n / p.NB <= (size_t)4 * p.L) return 0;
    // The TOP window is not uniform even for uniform scalars: the recoding folds s > r/2 to r - s, so its digit is at most
    // (r/2) >> off_top and each of its buckets holds n 2^off_top / (r/2) entries -- BLS12-377's r = 0x12ab... in 4-bit
    // windows: 0.43 n in one bucket against the average n / 8.  The tree is sized for that bucket too (the other short
    // windows at the top are at most twice the average: within piece_cmax's head-room).
    const unsigned off_top = p.nbits - window_len(p.nwins - 1, p.nwins, p.nbits);
    // Short scalars are not folded: the bound is 2^short_bits instead of r/2 (the plan's nbits = short_bits + 1: at most
    // half of the top window's digit range is in use, so its fullest bucket holds up to twice the average -- or all n when
    // the top window is that one bit alone).
    long double bound;
    if (short_bits) bound = ldexpl(1.0L, (int)short_bits);
    else {
        long double r = 0;
        for (int i = (int)scalar_words - 1; i >= 0; i--) r = r * 4294967296.0L + (long double)scalar_mod[i];
        bound = r / 2;
    }
    long double frac = ldexpl(1.0L, (int)off_top) / bound;
    if (frac > 1.0L) frac = 1.0L;
    const size_t top_pieces = (size_t)((long double)p.n * frac / p.L) + 2;
    const unsigned c = std::max(piece_cmax((size_t)p.n / p.NB / p.L + 1), piece_cmax_exact(top_pieces + top_pieces / 4 + 4));
    return c <= 1024 ? c : 0;
}

// wire points -> the field's own records.  G1 points in either wire layout at a 16-byte-aligned base: the coalesced form
// (msm_kernels.hpp k_convert_points_staged)
static inline msm_step route_convert(const msm_field& f, const msm_switches& sw, unsigned n, size_t stride, bool aligned16)
{
    msm_step s = msm_step();
    const size_t xy = 2 * (size_t)f.coord_bytes;
    if (f.g1_loose && (stride == xy || stride == xy + 8) && aligned16 && !sw.convert_per_lane)
        s.kernel = stride == xy ? MK_CONVERT_STAGED : MK_CONVERT_STAGED_FLAGGED;
    else
        s.kernel = stride > xy ? MK_CONVERT_FLAGGED : MK_CONVERT;
    s.gx = div_up(n, 256); s.gy = 1; s.block = 256; s.count = n;
    s.rd[0] = MB_POINTS; s.wr[0] = MB_CONV;
    return s;
}

// A chunked bucket-sum level of |nthr| work items.  Grids of at most one resident round (one wave per SIMD: LAT_LANES) are
// chains of dependent additions: at most one work-group of four waves per CU -- four waves per operation
// (msm_coop_kernels.hpp); between that and one resident round -- the chains of a work item on two (first level) / three
// waves; sums_one_lane: on one lane (the _lat kernels: no register cap, products in pairs).  Larger grids are work: two
// waves per SIMD.  G1 over the loosely-reduced fields only; the others have the plain kernels.
enum msm_sums_form { SUMS_PLAIN, SUMS_LAT, SUMS_PIPE, SUMS_COOP };
static inline msm_sums_form sums_form(size_t nthr, const msm_field& f, const msm_switches& sw)
{
    if (!f.g1_loose || nthr > LAT_LANES || sw.no_latency_sums) return SUMS_PLAIN;
    if (sw.no_coop) return SUMS_LAT;
    if (nthr <= COOP_LEVEL_MAX) return SUMS_COOP;
    return sw.sums_one_lane ? SUMS_LAT : SUMS_PIPE;
}
static inline msm_step& add_sums_level(msm_route& r, msm_kernel plain, unsigned pipe_block, size_t nthr, const msm_field& f, const msm_switches& sw)
{
    const msm_sums_form form = sums_form(nthr, f, sw);
    const msm_kernel k = (msm_kernel)(plain + form);
    if (form == SUMS_COOP) return r.add(k, div_up(nthr, 64), 1, COOP_NT);
    if (form == SUMS_PIPE) return r.add(k, div_up(nthr, 64), 1, pipe_block);
    return r.add(k, div_up(nthr, 256), 1, 256);
}

static inline msm_route make_route(const msm_plan& p, const msm_tunables& tune, const msm_field& f, const msm_call& c)
{
    msm_route r;
    const msm_switches& sw = tune.sw;
    const bool multi = p.G > 1;
    const bool coop = f.g1_loose && !sw.no_coop;

    if (!c.redo) {
        if (c.convert) r.steps[r.nsteps++] = route_convert(f, sw, p.n, c.stride, c.aligned16);
        // G2: one Fp2 component per wave (msm_g2c_kernels.hpp).  The default for the 14-limb base fields: BLS12-381 G2
        // 2^22 47.8 -> 40.2 ms, 2^20 15.3 -> 14.0; NOT for the 10-limb one, whose whole Fp2 bucket fits a lane at two
        // waves per SIMD already (alt_bn128 G2 2^22 21.6 -> 23.6 ms); profiles/r05_g2_coop_ab.log.
        // tune.g2_coop: 0 = that rule, 1 = wave pairs, 2 = one lane per addition (sppark_msm_g2_path).
        // (one step: a window group is grid row w0 ... w0 + wn of it)
        const bool by_pairs = f.pairs_built && (tune.g2_coop == 1 || (tune.g2_coop == 0 && f.pairs_default));
        msm_step& s = by_pairs ? r.add(MK_ACCUMULATE_G2C, div_up(p.chunks_per_win, 64), p.wpg, G2C_NT)
                               : r.add(c.flagged ? MK_ACCUMULATE_FLAGGED : MK_ACCUMULATE, div_up(p.chunks_per_win, 256), p.wpg, 256);
        s.rd[0] = c.convert ? MB_CONV : MB_POINTS; s.wr[0] = MB_KEY_A; s.wr[1] = MB_PT_A; s.count = p.n;
        r.front = r.nsteps;
    }

    // ---- small MSMs: the pieces of every bucket by a tree over the bucket's own pieces (msm_piece_kernels.hpp) ----
    // Where a bucket is cut into MORE runs than k_join_runs walks (n / NB > 4 L: up to 2^16 points), log2(cmax) launches of
    // one addition each replace the fan-in tree's eleven of up to three (2^16: 0.29 -> 0.09 ms, 2^12: 0.20 -> 0.08).  A
    // bucket with more than cmax pieces (skewed scalars) keeps its records and raises the flag; the fan-in tree is NOT
    // queued behind it -- ten launches that find nothing to do are 50 us -- but run afterwards by invoke() when the flag,
    // which comes back with the window sums, is set.  (One window group, whose offsets are all still there.)
    r.piece_cmax = c.may_defer ? piece_tree_cmax(p, sw, c.fb_n, f.scalar_mod, f.scalar_words, c.short_bits) : 0;
    // windows of up to 256 buckets (MSMs of up to 2^16 points): the subset sums straight from the buckets, then the parts of a
    // window (msm_coop_kernels.hpp k_bucket_small_bits_coop); needs the offsets of every window: one window group
    r.small_sums = coop && !multi && c.fb_n == 0 && p.NB <= SMALL_SUMS_MAX_NB && p.NB >= 2 && tune.K1 == 0 && tune.top == 0
                   && tune.K == 0 && !sw.no_latency_sums;
    // The flag of the piece tree on that path costs no launch of its own: it lives in a word that is ZERO between MSMs
    // (no memset), and the last kernel of the path -- k_bucket_top_sum_coop, which writes the window sums' wire image --
    // puts it behind the sums (one copy brings both to the host) and clears it.  (2^12: a 5 us fill with a 6 us gap in front
    // of the levels and a 5 us copy behind them, of a 0.39 ms MSM.)  Other paths: memset, levels, a copy of their own.
    r.flag_with_sums = r.small_sums && (r.piece_cmax != 0 || c.redo);
    const size_t nbuckets = (size_t)p.nwins * p.NB;
    if (r.piece_cmax && !c.redo) {
        const unsigned cm = r.piece_cmax;
        const msm_flag flag = r.flag_with_sums ? MF_SMALL : MF_SCRATCH;
        // the levels of few work items in one launch (k_piece_tail_coop)
        const unsigned t_fused = coop && !sw.piece_level_launches ? piece_tail_t0(nbuckets, cm, sw.piece_fuse_max) : ~0u;
        for (unsigned t = 0; (cm >> (t + 1)) >= 1; t++) {
            const size_t nthr = nbuckets * (cm >> (t + 1));
            msm_step* s;
            if (t == t_fused) {
                const unsigned lgGB = piece_tail_lgGB(cm, t);
                s = &r.add(MK_PIECE_TAIL_COOP, (unsigned)((nbuckets + ((size_t)1 << lgGB) - 1) >> lgGB), 1, COOP_NT);
                s->lgGB = lgGB;
            } else if (coop && nthr <= COOP_LEVEL_MAX) s = &r.add(MK_PIECE_LEVEL_COOP, div_up(nthr, 64), 1, COOP_NT);
            else s = &r.add(MK_PIECE_LEVEL, div_up(nthr, 256), 1, 256);
            s->t = t; s->last = (cm >> (t + 2)) == 0; s->flag = flag;
            s->rd[0] = MB_KEY_A; s->rd[1] = MB_PT_A; s->wr[0] = MB_BUCKETS;
            if (t == t_fused) break;
        }
        r.pieces = r.nsteps - r.front;
        r.piece_pending = true;
    }

    // ---- segmented record tree over the records of all windows -----------------------------
    if (!r.piece_pending) {
        size_t nrec = (size_t)2 * p.nwins * p.chunks_per_win;
        msm_buf ik = MB_KEY_A, ip = MB_PT_A, ok = MB_KEY_B, op = MB_PT_B;
        // segments of <= JOIN_WALK records (with uniform scalars: all of them) in one launch; the tree
        // below then only sees the records of longer segments and returns at once when there are none
        msm_flag skip = MF_NONE;
        // (not when the average bucket is longer than four runs: every segment is then longer than the join's walk
        // and the launch finds nothing to do -- below ~2^19 points)
        if (!sw.no_join && !c.redo && (size_t)p.n / p.NB <= (size_t)4 * p.L) {
            msm_step& s = r.add(MK_JOIN_RUNS, div_up(nrec / 2 + 1, 256), 1, 256);
            s.count = (unsigned)nrec; s.flag = MF_SCRATCH;
            s.rd[0] = MB_KEY_A; s.rd[1] = MB_PT_A; s.wr[0] = MB_KEY_C; s.wr[1] = MB_BUCKETS;
            ik = MB_KEY_C; skip = MF_SCRATCH;
        }
        const bool coop_tree = coop && !sw.no_narrow_end;
        for (; !r.overflow;) {
            const unsigned nthreads = div_up(nrec, p.F);
            msm_step* s;
            bool done = false;
            // from one work-group per CU on: four waves per addition (msm_coop_kernels.hpp)
            if (coop_tree && nthreads <= 64) { s = &r.add(MK_REDUCE_TAIL_COOP, 1, 1, COOP_NT); done = true; }
            else if (coop_tree && nthreads <= COOP_TREE_MAX) s = &r.add(MK_REDUCE_RUNS_COOP, div_up(nthreads, 64), 1, COOP_NT);
            // the narrow end: every remaining level in one launch
            // (the level kernels write into the OTHER buffer pair; there the pairs alternate from |ik| on)
            else if (nthreads <= REDUCE_TAIL_NT && !sw.no_narrow_end) { s = &r.add(MK_REDUCE_TAIL, 1, 1, REDUCE_TAIL_NT); done = true; }
            else { s = &r.add(MK_REDUCE_RUNS, div_up(nthreads, 256), 1, 256); s->last = done = nthreads == 1; }
            s->count = (unsigned)nrec; s->fan = p.F; s->nthreads = nthreads; s->flag = skip;
            s->rd[0] = ik; s->rd[1] = ip; s->wr[0] = ok; s->wr[1] = op;
            if (done) break;
            nrec = (size_t)2 * nthreads;
            std::swap(ik, ok); std::swap(ip, op);
        }
    }

    // ---- per-window weighted bucket sums ----------------------------------------------------
    if (r.small_sums) {
        const unsigned m = lg2_floor(p.NB);
        msm_step& b = r.add(MK_BUCKET_SMALL_BITS_COOP, m + 1, p.nwins, COOP_NT);
        b.m = m; b.rd[0] = MB_BUCKETS; b.wr[0] = MB_A2;
        msm_step& s = r.add(MK_BUCKET_TOP_SUM_COOP, p.nwins, 1, COOP_NT);         // (the wire image with it: no k_finalize)
        s.count = m + 1; s.flag = r.flag_with_sums ? MF_SMALL : MF_NONE;
        s.rd[0] = MB_A2; s.wr[0] = MB_W2; s.wr[1] = MB_SUMS;
        r.result = MB_W2; r.finalized = true;
    } else {
        unsigned nitems = p.NB / p.K1;
        msm_step& l1 = add_sums_level(r, MK_BUCKET_LEVEL1, 128, (size_t)p.nwins * nitems, f, sw);
        l1.fan = p.K1; l1.rd[0] = MB_BUCKETS; l1.wr[0] = MB_A1; l1.wr[1] = MB_W1;
        unsigned lgG = lg2_floor(p.K1);
        msm_buf ia = MB_A1, iw = MB_W1, oa = MB_A2, ow = MB_W2;
        while (nitems > 1 && !r.overflow) {
            // the top of the sums by bit-weighted subset sums (msm_kernels.hpp k_bucket_top_bits): depth, not work
            if (nitems <= (tune.top ? tune.top : BUCKET_TOP_MAX) && nitems >= 32 && (nitems & (nitems - 1)) == 0
                && (size_t)p.NB / p.K1 >= 32) {
                const unsigned m = lg2_floor(nitems);
                if (coop) {
                    // the tree and the doubling chains by four waves per operation (msm_coop_kernels.hpp)
                    // (a work-group per PIECE of a sum: msm_kernels.hpp bucket_top_piece; top_per_sum: per sum)
                    unsigned sb = 1, sp = 1;
                    if (!sw.top_per_sum) bucket_top_cut(nitems, COOP_NT, sb, sp);
                    const unsigned s1 = c.top_cut / 10, s2 = c.top_cut % 10;        // (sweeps only)
                    if (s1 >= 1 && s2 >= 1 && m * s1 + s2 <= 32 && nitems >= COOP_NT * s2) { sb = s1; sp = s2; }
                    msm_step& b = r.add(MK_BUCKET_TOP_BITS_COOP, m * sb + sp, p.nwins, COOP_NT, (unsigned)top_bits_coop_lds(f.words));
                    b.count = nitems; b.m = m; b.lgG = lgG; b.sb = sb; b.sp = sp;
                    b.rd[0] = ia; b.rd[1] = iw; b.wr[0] = oa;
                    msm_step& s = r.add(MK_BUCKET_TOP_SUM_COOP, p.nwins, 1, COOP_NT);     // (the wire image with it: no k_finalize)
                    s.count = m * sb + sp; s.rd[0] = oa; s.wr[0] = ow; s.wr[1] = MB_SUMS;
                    r.finalized = true;
                } else {
                    msm_step& b = r.add(MK_BUCKET_TOP_BITS, m + 1, p.nwins, BUCKET_TOP_NT, BUCKET_TOP_NT * f.bucket_bytes);
                    b.count = nitems; b.m = m; b.lgG = lgG;
                    b.rd[0] = ia; b.rd[1] = iw; b.wr[0] = oa;
                    msm_step& s = r.add(MK_BUCKET_TOP_SUM, p.nwins, 1, 32, 32 * f.bucket_bytes);
                    s.m = m; s.rd[0] = oa; s.wr[0] = ow;
                }
                std::swap(iw, ow);
                break;
            }
            const unsigned K = std::min(p.K, nitems);
            msm_step& s = add_sums_level(r, MK_BUCKET_LEVELN, 192, (size_t)p.nwins * (nitems / K), f, sw);
            s.count = nitems; s.fan = K; s.lgG = lgG;
            s.rd[0] = ia; s.rd[1] = iw; s.wr[0] = oa; s.wr[1] = ow;
            nitems /= K; lgG += lg2_floor(K);
            std::swap(ia, oa); std::swap(iw, ow);
        }
        r.result = iw;
    }
    // ---- the wire image of the window sums, where no step wrote it ---------------------------
    if (f.own_records && !r.finalized) {
        msm_step& s = r.add(MK_FINALIZE, div_up(p.nwins, 64), 1, 64);
        s.rd[0] = r.result; s.wr[0] = MB_SUMS;
    }
    return r;
}

} // namespace sppark_amd
