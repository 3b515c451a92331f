// The launch of one FRI call (include/sppark_amd_fri.h), decided in ONE pure function: make_fri_route(call) returns grid,
// tile and access style as data.  No HIP calls; api/fri_api.hpp launches what it returns and tests/emu/emu_fri.cpp runs the
// same geometry on the host.
//
// Geometry: a work-group of FRI_NT lanes takes tiles; a lane holds |acc| accesses of |pack| results per tile (pack = 16 bytes'
// worth of elements, or 1 in the element-wise instance), access u of lane t being chunk u * FRI_NT + t of the tile, so a tile
// is 2^out_lg = FRI_NT * acc * pack results.  A grid is at most FRI_WG_PER_CU work-groups per CU; a work-group strides over the
// tiles beyond that.
//
//   fold     a result is one group of 2^lg_arity inputs; a tile reads 64 bytes per lane where the arity leaves a whole access
//            of results (T = fri_tile_lg inputs for arity 1), more for the higher arities of the wide elements.  The grid is a
//            POWER OF TWO (it divides the tiles): a BITREV work-group b visits tile b + grid * bitrev(s) in step s, so that
//            the exponent of its twiddle goes up by one per step (fri_kernels.hpp).
//   domain   a result is one point; 64 bytes per lane and tile; the grid as fold's.
//   reduce   a result is one leaf; a lane owns |pack| consecutive leaves (columns layout, 16-byte accesses down the columns) or
//            one leaf (rows layout, 16-byte pieces along the leaf; element-wise instance); the weights are staged in LDS in
//            chunks of FRI_RED_CHUNK columns, and the grid strides over the leaves inside every chunk.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sppark_amd {

enum { FRI_NATURAL = 0, FRI_BITREV = 1 };
enum { FRI_OP_FOLD = 0, FRI_OP_DOMAIN = 1, FRI_OP_REDUCE = 2 };
enum { FRI_COLUMNS = 0, FRI_ROWS = 1 };

static constexpr unsigned FRI_NT = 256;             // lanes per work-group
static constexpr unsigned FRI_WG_PER_CU = 8;        // the grid's cap: work-groups per CU
static constexpr unsigned FRI_MAX_LG = 32;
static constexpr unsigned FRI_MAX_LG_ARITY = 3;
static constexpr unsigned FRI_RED_CHUNK = 512;      // weights staged in LDS at a time (16 KB of 32-byte elements)

// log2 of the elements 64 bytes per lane make: the tile of an arity-1 fold (inputs) and of domain (points)
static inline constexpr unsigned fri_tile_lg(size_t elem_bytes)
{   return elem_bytes <= 4 ? 12 : elem_bytes <= 8 ? 11 : elem_bytes <= 16 ? 10 : 9;   }
// elements per 16-byte access
static inline constexpr unsigned fri_pack(size_t elem_bytes) { return elem_bytes < 16 ? (unsigned)(16 / elem_bytes) : 1; }
// result accesses per lane and tile: what 64 bytes of inputs per lane leave, at least one
static inline constexpr unsigned fri_accesses(size_t elem_bytes, unsigned lg_arity, unsigned pack)
{
    const unsigned per_lane = (1u << fri_tile_lg(elem_bytes)) / FRI_NT;         // 16 / 8 / 4 / 2 elements
    return per_lane >> lg_arity >= pack ? (per_lane >> lg_arity) / pack : 1;
}
static inline constexpr unsigned fri_lg(unsigned v) { return v <= 1 ? 0 : 1 + fri_lg(v >> 1); }

struct fri_call {
    size_t elem_bytes = 8;          // the element the 16-byte accesses move: fold / domain: the library's field; reduce: the matrix's
    unsigned lg_n = 0;
    unsigned cus = 1;
    unsigned wg_per_cu = FRI_WG_PER_CU;     // (the emulation lowers it, so that a work-group takes many steps at small sizes)
    int op = FRI_OP_FOLD;
    unsigned lg_arity = 1;          // fold
    int order = FRI_NATURAL;        // fold, domain
    int layout = FRI_COLUMNS;       // reduce
    size_t width = 1;               // reduce
    bool aligned16 = true;          // every access of the call can be a 16-byte one (pointers and strides)
};

struct fri_route {
    unsigned grid = 0, block = FRI_NT;
    unsigned pack = 1;              // results per access (1: the element-wise instance)
    unsigned acc = 1;               // result accesses per lane and tile
    unsigned out_lg = 0;            // log2 results of a tile (reduce: leaves a work-group takes per step)
    unsigned tile_bits = 0;         // log2 tiles (fold, domain)
    unsigned grid_lg = 0;           // log2 grid (fold, domain)
    size_t tiles = 0;
    unsigned chunks = 0;            // reduce: passes over the leaves, one per FRI_RED_CHUNK weights
    bool vec = false;               // 16-byte accesses
    bool invalid = false;
};

static inline fri_route make_fri_route(const fri_call& c)
{
    fri_route r;
    const size_t es = c.elem_bytes;
    if ((es != 4 && es != 8 && es != 16 && es != 32) || c.lg_n > FRI_MAX_LG || c.op < FRI_OP_FOLD || c.op > FRI_OP_REDUCE) { r.invalid = true; return r; }
    const size_t cap = (size_t)std::max(c.cus, 1u) * std::max(c.wg_per_cu, 1u);
    if (c.op == FRI_OP_REDUCE) {
        if (c.width == 0 || (c.layout != FRI_COLUMNS && c.layout != FRI_ROWS)) { r.invalid = true; return r; }
        const size_t n = (size_t)1 << c.lg_n;
        r.vec = es >= 16 || c.aligned16;
        // columns: a lane owns a whole access of leaves, if there is one; rows: one leaf, read in 16-byte pieces
        r.pack = c.layout == FRI_COLUMNS && r.vec && n >= fri_pack(es) ? fri_pack(es) : 1;
        if (c.layout == FRI_COLUMNS && r.pack == 1 && es < 16) r.vec = false;
        r.acc = 1;
        r.out_lg = fri_lg(FRI_NT * r.pack);
        r.tiles = std::max<size_t>(n >> r.out_lg, 1);
        r.grid = (unsigned)std::min(r.tiles, cap);
        r.chunks = (unsigned)((c.width + FRI_RED_CHUNK - 1) / FRI_RED_CHUNK);
        return r;
    }
    const unsigned a = c.op == FRI_OP_FOLD ? c.lg_arity : 0;
    if ((c.op == FRI_OP_FOLD && (a < 1 || a > FRI_MAX_LG_ARITY || c.lg_n < a)) || (c.order != FRI_NATURAL && c.order != FRI_BITREV)) {
        r.invalid = true; return r;
    }
    const unsigned lg_m = c.lg_n - a;                                   // log2 results
    r.vec = es >= 16 || (c.aligned16 && ((size_t)1 << lg_m) >= fri_pack(es));
    r.pack = r.vec ? fri_pack(es) : 1;
    r.acc = fri_accesses(es, a, r.pack);
    r.out_lg = fri_lg(FRI_NT * r.acc * r.pack);
    r.tile_bits = lg_m > r.out_lg ? lg_m - r.out_lg : 0;
    r.tiles = (size_t)1 << r.tile_bits;
    // the largest power of two within tiles, cap and 2^12 (a work-group's index has three hexadecimal digits: fri_kernels.hpp)
    while (r.grid_lg < r.tile_bits && r.grid_lg < 12 && ((size_t)2 << r.grid_lg) <= cap) r.grid_lg++;
    r.grid = 1u << r.grid_lg;
    return r;
}

} // namespace sppark_amd
