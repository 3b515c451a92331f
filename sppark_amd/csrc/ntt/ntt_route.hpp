// The ROUTE of an NTT call: which kernels run, with which grids, LDS sizes, scalars and twiddle tables -- as data.
// A pure function of a few compile-time facts about the field (ntt_field), the plan's shape parameters (ntt_knobs) and
// the call at hand (ntt_call); no HIP call, no heap and no device pointers (the pointer members of ntt_pass stay null
// here).  ntt_driver.hpp ntt_engine::run() fetches the tables a route asks for and launches its steps one by one;
// tests/emu/emu_ntt.cpp runs the kernels' phase functions over the same steps and returns a route as integers, so that
// "what runs at size n" is checked at every size without a GPU (tests/test_ntt_route.py, against the launches an MI355X
// recorded).  The plan makers it calls (make_ntt_plan, make_ntt_lat_plan, make_r64_plan, r64_coset_mode) are host
// functions beside the kernels they describe, ntt_kernels.hpp / ntt_r64_kernels.hpp.
#pragma once
#include "ntt_r64_kernels.hpp"
#include <algorithm>
#include <cstddef>

namespace sppark_amd {

enum { NTT_NN = 0, NTT_NR = 1, NTT_RN = 2, NTT_RR = 3 };       // ntt/ntt.cuh:33
enum { NTT_FORWARD = 0, NTT_INVERSE = 1 };                     // ntt/ntt.cuh:34
enum { NTT_STANDARD = 0, NTT_COSET = 1 };                      // ntt/ntt.cuh:35

// what the route must know of the element type (ntt_engine<F>'s compile-time facts)
struct ntt_field {
    unsigned bytes;                     // sizeof(F)
    bool r64;                           // single-word field: the radix-64 plan (ntt_r64_kernels.hpp) exists
    unsigned two_adicity;
    bool gen_twiddles;                  // ntt_gen_twiddles<F>: a pass without a table generates its twiddles
    unsigned small_cap;                 // ntt_small_cap<F>: what k_ntt_small is compiled for
    unsigned bitrev_tile_bits;
};
template<class F> static inline ntt_field ntt_field_of()
{   return ntt_field{(unsigned)sizeof(F), sizeof(F) <= 8, F::TWO_ADICITY, ntt_gen_twiddles<F>::value, ntt_small_cap<F>::value, bitrev_tile_bits<F>::value};   }

// The plan's shape parameters.  A shipped library uses ntt_default_knobs(); a tuning build (-DSPPARK_TUNING) overrides
// fields from the environment once per process (ntt_driver.hpp ntt_engine::knobs(); the emulation sets them through its hooks).
struct ntt_knobs {
    unsigned smax, lgc, lgt;            // the register passes: stages per pass, log2 columns per tile row, log2 tile elements
    unsigned r64_min, r64_direct;       // the radix-64 plan: from this size on; largest single inter-pass table (log2)
    unsigned lat_smax;                  // the one-stage-per-round passes: stages per pass, 0 = the register passes
    int lat_lgc, lat_lgt;               // ... their tile shape, -1 = by size (make_ntt_lat_plan)
    unsigned coset_fold;                // 0: always the separate scaling launch
    unsigned small_max;                 // transforms up to this size: one launch of one work-group (k_ntt_small); 0 = never
    bool small_sized;                   // ... by the instance compiled for the size, where there is one
    unsigned packed_max;                // batched transforms up to this size: several columns per wave; 0 = never
    unsigned wide_table_lg;             // inter-pass tables up to 2^this entries: fields whose passes look twiddles up ...
    unsigned pass_table_max_lg;         // ... and fields whose passes can generate them
};
static inline ntt_knobs ntt_default_knobs(const ntt_field& f)
{
    ntt_knobs k;
    // columns per tile row (single-word fields: one 128-byte line; 256-bit fields: 16 elements =
    // 512 bytes, so that a 4-stage tile still has 64 register sub-transforms) / elements per LDS tile
    k.lgc = f.bytes == 4 ? 5 : 4;
    k.lgt = f.bytes == 4 ? 13 : f.bytes == 8 ? 12 : 10;
    // stages per pass.  256-bit elements: radix-4 x radix-4 (S = 4).  Larger register radices keep
    // 8 or 16 eight-word elements per lane (152 VGPRs, scratch) and measured slower in spite of
    // fewer passes: 2^24 in 2.8 ms with S = 4, 3.3 ms with S = 6 (tools/gpu_ntt_wide_knobs.py).
    // Round 3, with the twiddle tables and the <3, 3> kernel freed of its scratch use (its eight-element write-out loop
    // is above clang's #pragma-unroll budget; -mllvm -pragma-unroll-threshold=200000: 193 VGPRs, no scratch): 2.55 ms
    // with S = 6 against 2.54 with S = 4 on the same box, S = 5 2.81 -- a third fewer instructions and two passes less
    // buy nothing at two waves per SIMD (LDS: 256 B per lane).  Not instantiated.  profiles/r03_ntt_wide_stages.log
    k.smax = f.bytes > 8 ? 4 : 8;
    // the radix-64 plan: single-word fields, transforms of >= 2^12 elements; one inter-pass table up to 2^20 entries,
    // two small ones above
    k.r64_min = 12; k.r64_direct = 20;
    // Round 4: the 256-bit fields run passes of up to 8 stages with ONE butterfly per lane and stage and the tile in LDS
    // throughout (k_ntt_pass_lat, ntt_kernels.hpp): S/2 + 1 products per element for S stages instead of 3.75 for 4, half
    // the passes -- and half the dependent chain on the small, latency-bound sizes.  0 = the register passes above.
    k.lat_smax = f.bytes > 8 ? 8 : 0;
    k.lat_lgc = k.lat_lgt = -1;
    // a coset transform on a plan of k_ntt6 / k_ntt12 steps carries the powers of the coset generator in its tables and 64
    // constants (r64_coset_mode, ntt_r64_kernels.hpp): no separate scaling launch (2^24: 0.217 -> 0.19 ms)
    k.coset_fold = 1;
    // transforms up to this size run as one launch of one work-group: 2^11 for the single-word fields, 2^9 for the 256-bit
    // ones (at 2^10 their two one-stage-per-round launches are as fast as eight waves of 256-bit exchanges through
    // LDS: 17.7 against 17.8 us, profiles/r05_ntt_small_sized_ab.log)
    k.small_max = f.bytes > 8 ? f.small_cap - 1 : f.small_cap;
    k.small_sized = true;
    // batched transforms of up to this size run several columns per wave (k_ntt_small_packed, at most NTT_PACKED_MAX_LG = 6);
    // above it one work-group per column (DESIGN.md "Batched transforms")
    k.packed_max = NTT_PACKED_MAX_LG;
    // 256-bit elements: tables up to 2^24 entries (512 MB; every sub-problem of the pass reads its table once, the small
    // ones from L2 / the Infinity Cache).  The per-element alternative is a lo x hi product per twiddle: one of the ~3.5
    // products per element and pass.  BLS12-381 Fr 2^24 forward (profiles/r03_ntt_wide_tables.log): 2.80 ms without
    // tables, 2.43 with tables up to 2^16, 2.33 up to 2^20, 2.25 up to 2^24 -- even the table as large as the data pays,
    // the passes are bound by their products.
    k.wide_table_lg = 24;
    // fields that can generate their twiddles: tables of <= 2^16 elements (512 KB for Goldilocks): L2-resident
    k.pass_table_max_lg = 16;
    return k;
}

// one value per kernel template; its integer template arguments are fields of the step, DIF / INV the route's gs / inverse
enum ntt_kernel : unsigned char {
    NK_BITREV, NK_BITREV_TILED, NK_BITREV_TILED_VEC,    // k_bitrev<F>, k_bitrev_tiled<F, TB>, k_bitrev_tiled_vec<F, TB>
    NK_COSET,                                           // k_coset<F>
    NK_SMALL,                                           // k_ntt_small<F, INV, LGC>
    NK_SMALL_PACKED,                                    // k_ntt_small_packed<F, INV, LG>
    NK_PASS,                                            // k_ntt_pass<F, DIF, INV, R1, R2>
    NK_PASS_LAT,                                        // k_ntt_pass_lat<F, DIF, INV>
    NK_NTT6, NK_NTT12,                                  // k_ntt6 / k_ntt12<F, DIF, INV>
    NK_NTT12_LDE,                                       // k_ntt12<F, false, false, true>: reads the LDE's compact source
    // two steps the driver carries out through its helpers: lde_spread()'s launches over output ranges, and a (2D) copy
    NK_LDE_SPREAD, NK_COPY_OUT,
    NK_COUNT
};

// A twiddle table a step reads: enough to key it in the driver's cache and to build it.
enum ntt_table_family : unsigned char {
    NT_PASS,                            // k_pass_table: (lg_cur, S, scaled)
    NT_R64,                             // k_r64_table: (kind, lg_cur, scaled, cmode)
    NT_CZ,                              // k_r64_cz: (cmode)
    NT_CROW                             // k_pass_crow: (cmode, S)
};
struct ntt_table_req {
    ntt_table_family family;
    unsigned kind, lg_cur, S, cmode;
    bool scaled;
    size_t count;                       // elements
    // the cache key behind (device, direction).  W = w_n^(n / n_cur) is the primitive n_cur-th root whatever the transform
    // size n, so an unscaled table without coset powers is shared by every size; one that carries 1/n or powers of the
    // coset generator belongs to one size and its key ends in lg n.
    int key_family; unsigned key_a, key_b, key_c;
};
static inline ntt_table_req ntt_pass_table_req(unsigned lg, unsigned lg_cur, unsigned S, bool scaled)
{   return ntt_table_req{NT_PASS, 0, lg_cur, S, 0, scaled, (size_t)1 << lg_cur, 0, lg_cur, S, scaled ? lg : 0u};   }
static inline ntt_table_req ntt_r64_table_req(unsigned lg, unsigned kind, unsigned lg_cur, bool scaled, unsigned cmode)
{
    if (cmode == 2 && kind == 2) cmode = 0;                     // (no row-only part: the plain table)
    const size_t count = kind == 0 ? (size_t)1 << lg_cur : kind == 1 ? (size_t)1 << (lg_cur - 6) : 4096;
    if (cmode) return ntt_table_req{NT_R64, kind, lg_cur, 0, cmode, scaled, count, 1 + 10 * (int)cmode, kind, lg_cur, lg | (scaled ? 256u : 0u)};
    return ntt_table_req{NT_R64, kind, lg_cur, 0, 0, scaled, count, 1, kind, lg_cur, scaled ? lg : 0u};
}
static inline ntt_table_req ntt_cz_req(unsigned lg, unsigned cmode)
{   return ntt_table_req{NT_CZ, 0, 0, 0, cmode, false, 64, 2, cmode, 0u, lg};   }
static inline ntt_table_req ntt_crow_req(unsigned lg, unsigned cmode, unsigned S)
{   return ntt_table_req{NT_CROW, 0, 0, S, cmode, false, (size_t)1 << S, 3, cmode, S, lg};   }

struct ntt_step {
    ntt_kernel kernel;
    unsigned char R1, R2;               // NK_PASS
    unsigned char LGC;                  // NK_SMALL: the instance's size, 0 = the run-time-size one
    unsigned char LG;                   // NK_SMALL_PACKED
    unsigned gx, gy, block, lds;        // grid in work-groups (gy: a row per column; NK_SMALL_PACKED: per work-group of columns), dynamic LDS bytes
    // the scalars that differ from step to step
    ntt_pass pass;                      // NK_PASS / NK_PASS_LAT (its pointers null: the driver fills them by role)
    unsigned lg_cur;                    // NK_NTT6 / NK_NTT12*
    unsigned flags;                     // NK_SMALL / NK_SMALL_PACKED: ntt_small_flags
    int bitrev;                         // NK_COSET: bit-reversed exponents
    size_t spread_in_stride;            // NK_LDE_SPREAD: elements between the columns of the source
    // what it needs by role: indices into ntt_route::tables, -1 = null
    signed char tw, t1, t2, cz, crow, pass_tw;
    bool lde_src;                       // reads the LDE's compact source (NK_NTT12_LDE, NK_LDE_SPREAD)
    bool lde_out;                       // stores to the LDE's output (NK_NTT12 as the last step, NK_COPY_OUT)
    unsigned stages;                    // butterfly stages the step performs
    bool scales;                        // multiplies by 1/n (itself, or through a scaled table)
};

// the call at hand
enum ntt_lde_mode : unsigned char { NL_NONE, NL_SPREAD, NL_OUT };
struct ntt_call {
    unsigned lg = 0;
    int order = NTT_NN, direction = NTT_FORWARD, type = NTT_STANDARD;
    size_t batch = 1;                   // columns still to do: the route covers the first ntt_route::cols of them
    size_t col_stride = 0;              // elements between columns
    size_t max_grid_y = 65535;          // the device's limit on the grid's y dimension
    bool aligned16 = true;              // the first column and (more than one column) the column stride are 16-byte aligned
    // sppark_lde's hand-over.  NL_SPREAD (its forward RN transform): the input is still the compact 2^lg_domain coefficients,
    // bit-reversed order, unshifted.  NL_OUT (its inverse NR transform): the result goes to a second buffer.
    ntt_lde_mode lde = NL_NONE;
    unsigned lg_domain = 0, lg_blowup = 0;
    // the device had no room for a table: without the radix-64 plan / without the table that carries 1/n
    bool no_r64 = false, no_scaled_table = false;
};

struct ntt_route {
    // The longest: NN forward coset, unfolded = bit reversal + k_coset + 16 passes (what an ntt_plan holds), RR inverse coset
    // = 16 passes + k_coset + bit reversal: 18; the LDE's transforms, spread + 16 passes / 16 passes + copy: 17.  (A shipped
    // library has at most 4 passes: 2^32 in passes of 8 stages, or as 8 + 6 + 6 + 12.)
    static constexpr unsigned CAP = 18;
    // a table per pass of a 16-pass plan; the radix-64 plan (at most 4 steps): two per step + cz + crow + the top pass's
    static constexpr unsigned TCAP = 16;
    ntt_step steps[CAP];
    unsigned nsteps = 0;
    ntt_table_req tables[TCAP];
    unsigned ntables = 0;
    bool overflow = false;              // (cannot happen: see CAP; the tests hold it to that)
    bool invalid = false;               // the call is refused: hipErrorInvalidValue
    size_t cols = 0;                    // columns this route covers (<= ntt_launch_cols); the caller routes the rest again
    bool gs = false, inverse = false;   // the DIF network / the inverse transform: DIF and INV of every transform kernel
    bool r64 = false;                   // the radix-64 plan
    unsigned cmode = 0;                 // the coset transform is folded into the passes (r64_coset_mode)
    bool lde_fused = false;             // the LDE's spread rides in the first k_ntt12

    ntt_step& add(ntt_kernel k, unsigned gx, unsigned gy, unsigned block, unsigned lds = 0)
    {
        if (nsteps == CAP) { overflow = true; nsteps--; }
        ntt_step& s = steps[nsteps++];
        s = ntt_step();
        s.kernel = k; s.gx = gx; s.gy = gy; s.block = block; s.lds = lds;
        s.tw = s.t1 = s.t2 = s.cz = s.crow = s.pass_tw = -1;
        return s;
    }
    signed char want(const ntt_table_req& q)
    {
        if (ntables == TCAP) { overflow = true; ntables--; }
        tables[ntables] = q;
        return (signed char)ntables++;
    }
};

// columns one launch covers: the grid's y dimension, times the columns of a work-group of k_ntt_small_packed
static inline size_t ntt_launch_cols(const ntt_knobs& k, unsigned lg, size_t max_grid_y)
{
    const size_t rows = std::max<size_t>(max_grid_y, 1);
    return lg >= 1 && lg <= k.packed_max && lg <= k.small_max ? rows << (9 - lg) : rows;
}

// the inter-pass twiddle table of a pass on sub-problems of 2^lg_cur elements (built once per (device, direction, pass
// shape); none: the pass generates its twiddles / looks them up per element)
static inline bool ntt_has_pass_table(const ntt_field& f, const ntt_knobs& k, unsigned lg_cur, unsigned S)
{   return !(lg_cur > (f.gen_twiddles ? k.pass_table_max_lg : k.wide_table_lg) || lg_cur <= S || S / 2 == 0);   }

// in-place bit-reversal permutation of |cols| columns (NN and RR orders; ntt/ntt.cuh:44-79)
static inline ntt_step ntt_route_bitrev(const ntt_field& f, unsigned lg, size_t cols, bool aligned16)
{
    ntt_step s = ntt_step();
    const unsigned TB = f.bitrev_tile_bits;
    const size_t n = (size_t)1 << lg;
    s.gy = (unsigned)cols; s.block = 256;
    s.tw = s.t1 = s.t2 = s.cz = s.crow = s.pass_tw = -1;
    if (lg >= 2 * TB + 1) {
        // 16-byte accesses for the single-word fields (any 16-byte aligned buffer; a view at an odd element offset
        // takes the element-wise tiles) -- in a batch, only when every column starts 16-byte aligned
        s.kernel = f.bytes <= 8 && aligned16 ? NK_BITREV_TILED_VEC : NK_BITREV_TILED;
        s.gx = (unsigned)(n >> (2 * TB));
        s.lds = (unsigned)(2 * (((size_t)(1u << TB) + 1) << TB) * f.bytes);
    } else {
        s.kernel = NK_BITREV;
        s.gx = (unsigned)((n + 255) / 256);
    }
    return s;
}

static inline ntt_route make_ntt_route(const ntt_field& f, const ntt_knobs& k, const ntt_call& c)
{
    ntt_route r;
    const unsigned lg = c.lg;
    r.cols = std::min(c.batch, ntt_launch_cols(k, lg, c.max_grid_y));
    const unsigned ncol = (unsigned)r.cols;
    auto spread = [&](size_t in_stride) { ntt_step& s = r.add(NK_LDE_SPREAD, 0, ncol, 256); s.lde_src = true; s.spread_in_stride = in_stride; };
    auto copy_out = [&] { r.add(NK_COPY_OUT, 0, ncol, 0).lde_out = true; };
    if (lg == 0) {                                              // ntt/ntt.cuh:220-221 (one element: the hand-over of sppark_lde still happens)
        if (c.lde == NL_OUT) copy_out();
        else if (c.lde == NL_SPREAD) spread(1);
        return r;
    }
    if (lg > f.two_adicity || c.order < 0 || c.order > 3) { r.invalid = true; return r; }
    const bool inverse = r.inverse = c.direction == NTT_INVERSE;
    const bool coset = c.type == NTT_COSET;
    const size_t n = (size_t)1 << lg;
    bool final_out = c.lde == NL_OUT, lde = c.lde == NL_SPREAD;

    // up to 2^11 elements (256-bit fields: 2^9): the whole transform -- permutations, coset powers and 1/n included -- by one
    // work-group in one launch (k_ntt_small, ntt_kernels.hpp)
    if (lg <= k.small_max) {
        if (lde) spread((size_t)1 << c.lg_domain);
        const unsigned flags = ntt_small_flags(c.order, inverse, coset);
        r.gs = (flags & NTT_SMALL_GS) != 0;
        if (r.cols > 1 && lg <= k.packed_max) {                 // several columns per wave (k_ntt_small_packed)
            ntt_step& s = r.add(NK_SMALL_PACKED, 1, (unsigned)((r.cols + (256u >> (lg - 1)) - 1) >> (9 - lg)), 256);
            s.LG = (unsigned char)std::min(lg, NTT_PACKED_MAX_LG); s.flags = flags; s.stages = lg; s.scales = inverse;
        } else {
            const unsigned lanes = (unsigned)std::max<size_t>(64, n / 2);
            // (LDS: the exchanges across waves, ntt_rx_regroup)
            ntt_step& s = r.add(NK_SMALL, 1, ncol, lanes, lanes > 64 ? (unsigned)(2 * (size_t)lanes * f.bytes) : 0);
            // (single-word fields: the sizes 2^8 ... 2^11 have their own instance, compiled for that size)
            s.LGC = (unsigned char)(f.bytes <= 8 && k.small_sized && lg >= 8 && lg <= 11 ? lg : 0);
            s.flags = flags; s.stages = lg; s.scales = inverse;
        }
        if (final_out) copy_out();
        return r;
    }

    bool bitrev;
    switch (c.order) {
        case NTT_NN: r.steps[r.nsteps++] = ntt_route_bitrev(f, lg, r.cols, c.aligned16);
                     bitrev = true;  r.gs = false; break;
        case NTT_NR: bitrev = false; r.gs = true;  break;
        case NTT_RN: bitrev = true;  r.gs = false; break;
        default:     bitrev = true;  r.gs = true;  break;
    }
    const bool gs = r.gs;
    // the radix-64 plan and, on it, a folded coset transform
    r64_plan rp; rp.nsteps = 0;
    if (f.r64 && lg >= 12 && lg >= k.r64_min && !c.no_r64) {
        rp = make_r64_plan(lg);
        r.r64 = true;
        r.cmode = k.coset_fold ? r64_coset_mode(rp, gs, inverse, coset && c.order != NTT_RR) : 0;
    }
    const unsigned cmode = r.cmode;
    // sppark_lde: the spread + coset shift inside the first step where that is k_ntt12 on a forward RN transform with at
    // most 8 positions per coefficient; otherwise as a launch of its own, now
    if (lde) {
        r.lde_fused = r.r64 && !gs && !inverse && c.order == NTT_RN && !coset && rp.step[rp.nsteps - 1].kind == 2
                   && c.lg_blowup >= 1 && c.lg_blowup <= 3 && c.lg_domain + c.lg_blowup == lg;
        if (!r.lde_fused) spread((size_t)1 << c.lg_domain);
    }
    const unsigned egrid = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 22);   // (k_coset strides past 2^30)
    if (!inverse && coset && !cmode) r.add(NK_COSET, egrid, ncol, 256).bitrev = (int)bitrev;

    const bool lat = k.lat_smax != 0;
    ntt_plan pl;
    if (r.r64) pl.npass = rp.nsteps;
    else {
        if ((lg + (lat ? k.lat_smax : k.smax) - 1) / (lat ? k.lat_smax : k.smax) > 16) { r.invalid = true; return r; }   // (more passes than an ntt_plan holds)
        pl = lat ? make_ntt_lat_plan(lg, k.lat_smax, k.lat_lgc, k.lat_lgt) : make_ntt_plan(lg, k.lgc, k.lgt, k.smax);
    }
    // 1/n of an inverse transform: carried by the table of the tabled pass on the smallest sub-problems when the
    // plan has one (a product per element saved), applied by the last pass otherwise.  (The radix-64 plan folds it
    // into the table of its own last step.)
    int scale_pass = -1;
    if (inverse && !r.r64 && !c.no_scaled_table) {
        unsigned best = ~0u;
        for (unsigned i = 0; i < pl.npass; i++) {
            const ntt_pass& q = pl.pass[gs ? i : pl.npass - 1 - i];
            if (ntt_has_pass_table(f, k, q.lg_cur, q.S) && q.lg_cur < best) { best = q.lg_cur; scale_pass = (int)i; }
        }
    }
    const signed char cz = r.r64 && cmode ? r.want(ntt_cz_req(lg, cmode)) : (signed char)-1;    // (fetched with the plan, read or not)
    for (unsigned i = 0; i < pl.npass; i++) {
        const bool last = i == pl.npass - 1;
        ntt_pass P;
        signed char crow = -1;
        if (r.r64) {
            const r64_step st = rp.step[gs ? i : rp.nsteps - 1 - i];
            if (st.kind != 0) {
                const bool fused = r.lde_fused && i == 0;
                ntt_step& s = r.add(fused ? NK_NTT12_LDE : st.kind == 1 ? NK_NTT6 : NK_NTT12, (unsigned)(n >> 12), ncol, 512, f.bytes << 12);
                s.lg_cur = st.lg_cur; s.stages = st.S; s.lde_src = fused;
                const bool scaled = s.scales = inverse && last;
                // the coset powers in the tables of the step on the whole transform (natural exponents) / of every step
                // (bit-reversed exponents), the 64 constants in that step / in k_ntt12
                const unsigned cm = cmode == 1 && st.lg_cur != lg ? 0 : cmode;
                if (cmode == 2 ? st.kind == 2 : (cmode == 1 && st.lg_cur == lg)) s.cz = cz;
                if (st.kind == 2 || st.lg_cur <= k.r64_direct) s.tw = r.want(ntt_r64_table_req(lg, 0, st.lg_cur, scaled, cm));
                else { s.t1 = r.want(ntt_r64_table_req(lg, 1, st.lg_cur, scaled, cm)); s.t2 = r.want(ntt_r64_table_req(lg, 2, st.lg_cur, false, cm)); }
                if (final_out && last && st.kind == 2 && gs) { s.lde_out = true; final_out = false; }
                continue;
            }
            P.lg_cur = st.lg_cur; P.S = st.S; P.lgC = k.lgc; P.lgG = 0;         // a strided pass above >= 12 further stages
            // (a folded coset transform: the pass takes its share as 2^S row constants, g^(row << lgQ) / g^(rev_S(row)))
            P.cmode = cmode; P.crow = P.cg_lo = P.cg_hi = nullptr; P.cg_h = 0;
            if (cmode) crow = r.want(ntt_crow_req(lg, cmode, st.S));
        } else {
            P = pl.pass[gs ? i : pl.npass - 1 - i];
        }
        const bool scale_here = inverse && scale_pass == (int)i;
        P.apply_scale = inverse && last && scale_pass < 0;
        const size_t tile_elems = (size_t)1 << (P.lgG + P.S + P.lgC);
        const unsigned tiles = (unsigned)(n / tile_elems);
        ntt_step* s;
        if (lat && !r.r64) {                                    // one butterfly per lane and stage, the tile in LDS throughout
            const size_t lat_lds = tile_elems * f.bytes;
            if (lat_lds > 64 * 1024) { r.invalid = true; return r; }            // (only a tuning build can ask for such a tile)
            s = &r.add(NK_PASS_LAT, tiles, ncol, (unsigned)std::min<size_t>(std::max<size_t>(tile_elems / 2, 64), 1024), (unsigned)lat_lds);
        } else {
            // one lane per register sub-transform: a tile has 2^(lgG + R1 + lgC) of them in its
            // larger round (small tiles of wide elements would leave most of 256 lanes idle)
            const unsigned groups = 1u << (P.lgG + (P.S + 1) / 2 + P.lgC);
            s = &r.add(NK_PASS, tiles, ncol, groups >= 512 ? 512 : groups <= 64 ? 64 : groups, (unsigned)(ntt_lds_elems(P) * f.bytes));
            s->R1 = (unsigned char)((P.S + 1) / 2); s->R2 = (unsigned char)(P.S / 2);
        }
        s->pass = P; s->crow = crow; s->stages = P.S; s->scales = scale_here || P.apply_scale;
        if (ntt_has_pass_table(f, k, P.lg_cur, P.S)) s->pass_tw = r.want(ntt_pass_table_req(lg, P.lg_cur, P.S, scale_here));
    }
    if (inverse && coset && !cmode) r.add(NK_COSET, egrid, ncol, 256).bitrev = (int)!bitrev;
    if (c.order == NTT_RR) { if (r.nsteps == ntt_route::CAP) r.overflow = true; else r.steps[r.nsteps++] = ntt_route_bitrev(f, lg, r.cols, c.aligned16); }
    if (final_out) copy_out();                                  // (no step stored there)
    return r;
}

} // namespace sppark_amd
