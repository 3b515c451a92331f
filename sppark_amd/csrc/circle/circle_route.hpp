// The kernel sequence of one circle transform (or one launch group of a batch), decided in ONE pure function:
// make_circle_route(knobs, call) returns the steps as data -- kernel, grid, block, LDS bytes, layers, tables wanted, which
// step scales.  No HIP calls; circle_driver.hpp launches what it returns and tests/emu/emu_circle.cpp runs the same
// steps on the host.
//
// Passes: the lowest min(k, low_max) layers are one pass on contiguous tiles; the k - low_max layers above them are cut
// into ceil((k - low_max) / high_max) passes of nearly equal depth, each on tiles of [2^S rows] x [2^(tile_lg - S)
// columns].  Launches: 1 for k <= low_max, else 1 + ceil((k - low_max) / high_max); NATURAL order adds one bit-reversal.
// Forward runs the passes from the top layers down, inverse from the bottom up; the inverse's last pass multiplies by 1/n.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sppark_amd {

enum { CIRCLE_EVALS_BITREV = 0, CIRCLE_EVALS_NATURAL = 1 };
enum { CIRCLE_FORWARD = 0, CIRCLE_INVERSE = 1 };

// tile edge (bits) of the tiled bit reversal for 4-byte elements: ntt_kernels.hpp bitrev_tile_bits (the driver asserts they agree)
static constexpr unsigned CIRCLE_BITREV_TILE_BITS = 6;

struct circle_knobs {
    unsigned low_max = 12;          // layers of the pass on the lowest layers (its tile: 2^low_max contiguous elements)
    unsigned high_max = 8;          // layers of a pass above it
    unsigned tile_lg = 12;          // log2 elements of a tile (16 KB of data + at most 16 KB of twiddles in LDS)
    unsigned block = 256;           // lanes of a work-group
    unsigned cache_max_lg = 24;     // inverse-twiddle tables L_m / Y_m are kept per device for m <= this (64 MB in all);
                                    // larger ones live in the call's scratch
    unsigned lds_cap = 65536;
    unsigned bitrev_tile_bits = CIRCLE_BITREV_TILE_BITS;
};

enum circle_kernel : unsigned char { CK_PASS, CK_BITREV, CK_BITREV_TILED, CK_BITREV_TILED_VEC };

struct circle_table_req {
    unsigned m;             // the table's size parameter: 2^(m-2) entries
    bool y;                 // Y_m (the y-layer of size m) or L_m (x-layers)
    bool cached;            // kept per device, or part of the call's scratch
    size_t count;
};

struct circle_step {
    circle_kernel kernel;
    unsigned gx, gy, block, lds;
    unsigned lg;                        // the column size this step works on
    unsigned b_lo, S, lgC, lgT;         // CK_PASS
    bool inverse, scales, vec;
    unsigned pad_lg;                    // CK_PASS: positions >= 2^pad_lg are read as zero (>= lg: none)
    signed char table[12];              // CK_PASS, inverse: index into circle_route::tables per layer of the pass, -1 none
};

struct circle_call {
    unsigned lg = 0;
    int order = CIRCLE_EVALS_BITREV, direction = CIRCLE_FORWARD;
    size_t batch = 1;
    size_t max_grid_y = 65535;      // the device's limit on the grid's y dimension
    bool aligned16 = true;          // every column starts 16-byte aligned
    unsigned pad_lg = 32;           // forward: the column holds 2^pad_lg coefficients, the rest counts as zero (the LDE)
};

struct circle_route {
    static constexpr unsigned CAP = 8, TCAP = 32;
    circle_step steps[CAP];
    circle_table_req tables[TCAP];
    unsigned nsteps = 0, ntables = 0;
    size_t cols = 0;                // columns one launch group covers; a larger batch is split by the driver
    size_t scratch_entries = 0;     // elements of the uncached tables (at most 2^lg)
    bool needs_points = false;      // forward passes: the 4096-entry point tables
    bool invalid = false;
};

static inline unsigned circle_lg_ceil(size_t v) { unsigned l = 0; while (((size_t)1 << l) < v) l++; return l; }

// how many columns of 2^lg elements one work-group of the low pass holds (log2), for a batch of |batch|
static inline unsigned circle_pack_lg(const circle_knobs& k, unsigned lg, size_t batch)
{   return lg >= k.tile_lg || lg > k.low_max ? 0 : std::min(k.tile_lg - lg, circle_lg_ceil(std::max<size_t>(batch, 1)));   }

static inline size_t circle_launch_cols(const circle_knobs& k, unsigned lg, int order, size_t batch, size_t max_grid_y)
{
    const size_t rows = std::max<size_t>(max_grid_y, 1);
    // (the bit-reversal of the NATURAL order takes one grid row per column)
    return order == CIRCLE_EVALS_NATURAL ? rows : rows << circle_pack_lg(k, lg, batch);
}

static inline circle_step circle_route_bitrev(const circle_knobs& k, unsigned lg, size_t cols, bool aligned16)
{
    circle_step s = circle_step();
    const unsigned TB = k.bitrev_tile_bits;
    s.lg = lg; s.gy = (unsigned)cols; s.block = 256; s.pad_lg = 32;
    for (auto& t : s.table) t = -1;
    if (lg >= 2 * TB + 1) {
        s.kernel = aligned16 ? CK_BITREV_TILED_VEC : CK_BITREV_TILED;
        s.gx = (unsigned)(((size_t)1 << lg) >> (2 * TB));
        s.lds = (unsigned)(2 * (((size_t)(1u << TB) + 1) << TB) * 4);
    } else {
        s.kernel = CK_BITREV;
        s.gx = (unsigned)((((size_t)1 << lg) + 255) / 256);
    }
    return s;
}

static inline circle_route make_circle_route(const circle_knobs& k, const circle_call& c)
{
    circle_route r;
    const unsigned lg = c.lg;
    const bool inverse = c.direction == CIRCLE_INVERSE;
    if (lg > 30 || (c.order != CIRCLE_EVALS_BITREV && c.order != CIRCLE_EVALS_NATURAL) || (c.direction != CIRCLE_FORWARD && !inverse)
        || k.low_max < 2 || k.low_max > 12 || k.low_max > k.tile_lg || k.high_max < 1 || k.high_max + 4 > k.tile_lg || k.tile_lg > 12) {
        r.invalid = true; return r;
    }
    if (lg == 0 || c.batch == 0) return r;
    r.cols = std::min(c.batch, circle_launch_cols(k, lg, c.order, c.batch, c.max_grid_y));
    const unsigned pack = circle_pack_lg(k, lg, r.cols);

    // the passes, lowest layers first
    struct span { unsigned b_lo, S; } spans[circle_route::CAP];
    unsigned np = 0;
    spans[np++] = span{0, std::min(lg, k.low_max)};
    if (lg > k.low_max) {
        const unsigned rem = lg - k.low_max, nh = (rem + k.high_max - 1) / k.high_max;
        unsigned b = k.low_max;
        for (unsigned i = 0; i < nh; i++) { const unsigned S = rem / nh + (i < rem % nh ? 1 : 0); spans[np++] = span{b, S}; b += S; }
    }
    if (np + 1 > circle_route::CAP) { r.invalid = true; return r; }

    if (inverse && c.order == CIRCLE_EVALS_NATURAL) r.steps[r.nsteps++] = circle_route_bitrev(k, lg, r.cols, c.aligned16);
    for (unsigned i = 0; i < np; i++) {
        const span sp = spans[inverse ? i : np - 1 - i];
        circle_step s = circle_step();
        s.kernel = CK_PASS; s.lg = lg; s.b_lo = sp.b_lo; s.S = sp.S; s.inverse = inverse; s.block = k.block;
        for (auto& t : s.table) t = -1;
        if (sp.b_lo == 0) {
            s.lgC = 0; s.lgT = sp.S + pack;
            s.gx = (unsigned)(((size_t)1 << lg) >> sp.S);
            s.gy = (unsigned)((r.cols + (((size_t)1 << pack) - 1)) >> pack);
        } else {
            s.lgC = std::min(k.tile_lg - sp.S, sp.b_lo); s.lgT = sp.S + s.lgC;      // (the columns are bits below b_lo)
            s.gx = (unsigned)(((size_t)1 << lg) >> s.lgT);
            s.gy = (unsigned)r.cols;
        }
        // the tile (one pad word per 16 elements, circle_kernels.hpp circle_lds_index) and its 2^S twiddles
        s.lds = (unsigned)((((size_t)1 << s.lgT) + (((size_t)1 << s.lgT) >> 4) + ((size_t)1 << s.S)) * 4);
        s.scales = inverse && i == np - 1;
        // the padding rides in the FIRST forward pass, which reads every element of the column once
        s.pad_lg = !inverse && i == 0 && c.pad_lg < lg ? c.pad_lg : 32;
        s.vec = c.aligned16 && lg >= 2 && (s.pad_lg >= 32 || s.pad_lg >= 2);
        if (inverse)
            for (unsigned lb = 0; lb < sp.S; lb++) {
                const unsigned b = sp.b_lo + lb, m = b ? lg - b + 1 : lg;
                if (m < 2) continue;                                        // lg = 1: the kernel knows 1 / y(g_2) = -1
                circle_table_req q;
                q.m = m; q.y = b == 0; q.cached = m <= k.cache_max_lg; q.count = (size_t)1 << (m - 2);
                if (r.ntables >= circle_route::TCAP) { r.invalid = true; return r; }
                if (!q.cached) r.scratch_entries += q.count;
                s.table[lb] = (signed char)r.ntables;
                r.tables[r.ntables++] = q;
            }
        else r.needs_points = true;
        if (s.lds > k.lds_cap || s.gy > c.max_grid_y) { r.invalid = true; return r; }
        r.steps[r.nsteps++] = s;
    }
    if (!inverse && c.order == CIRCLE_EVALS_NATURAL) r.steps[r.nsteps++] = circle_route_bitrev(k, lg, r.cols, c.aligned16);
    return r;
}

} // namespace sppark_amd
