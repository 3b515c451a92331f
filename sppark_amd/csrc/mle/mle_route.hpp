// The launches of one multilinear-table call (include/sppark_amd_mle.h), decided in ONE pure function: make_mle_route(call)
// returns the steps as data -- kernel, grid, tile, variables bound, scratch elements, access style.  No HIP calls;
// api/mle_api.hpp launches what it returns and tests/emu/emu_mle.cpp runs the same steps on the host.
//
// Geometry: a work-group of MLE_NT lanes takes tiles of 2^T elements, 64 bytes per lane: T = 12 / 11 / 10 / 9 for elements of
// 4 / 8 / 16 / 32 bytes (mle_tile_lg).  A grid is at most MLE_WG_PER_CU work-groups per CU; a work-group strides over the
// tiles beyond that.
//
//   fold      one launch; a tile is 2^T elements read (2^(T-1) pairs), one variable bound
//   evaluate  ceil(lg_n / T) launches: as many passes over whole tiles of T variables as fit, then one over the rest; a pass
//             writes one element per tile into the call's scratch, the last one the result
//   eq        one launch; a tile is 2^min(lg_n, T) elements written
//   round     two launches: one slab row of |rows| sums per work-group, then one work-group that sums the rows
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sppark_amd {

enum { MLE_LOW = 0, MLE_HIGH = 1 };
enum { MLE_OP_FOLD = 0, MLE_OP_EVALUATE = 1, MLE_OP_EQ = 2, MLE_OP_ROUND = 3 };
enum mle_kernel : unsigned char { MK_FOLD, MK_BIND, MK_EQ, MK_ROUND, MK_ROUND_SUM };

static constexpr unsigned MLE_NT = 256;             // lanes per work-group
static constexpr unsigned MLE_WG_PER_CU = 8;        // the grid's cap: work-groups per CU
static constexpr unsigned MLE_MAX_LG = 32;

// log2 of the elements of a tile: 64 bytes per lane
static inline constexpr unsigned mle_tile_lg(size_t elem_bytes)
{   return elem_bytes <= 4 ? 12 : elem_bytes <= 8 ? 11 : elem_bytes <= 16 ? 10 : 9;   }
// elements per 16-byte access
static inline constexpr unsigned mle_pack(size_t elem_bytes) { return elem_bytes < 16 ? (unsigned)(16 / elem_bytes) : 1; }

struct mle_call {
    size_t elem_bytes = 8;
    unsigned lg_n = 0;
    unsigned cus = 1;
    int op = MLE_OP_FOLD;
    unsigned rows = 0;              // round: the d + 1 sums
    bool aligned16 = true;          // every buffer of the caller's starts 16-byte aligned
};

struct mle_step {
    mle_kernel kernel;
    unsigned grid, block;
    unsigned tile_lg;               // log2 elements of a tile of this step
    unsigned vars;                  // variables this step binds (eq: expands)
    unsigned var_base;              // the first of them (bind)
    size_t tiles;                   // tiles of the step (round sum: rows to add)
    size_t writes;                  // elements it writes into the call's scratch
    bool vec;                       // 16-byte accesses (false: the element-wise instance)
};

struct mle_route {
    static constexpr unsigned CAP = 8;
    mle_step steps[CAP];
    unsigned nsteps = 0;
    size_t scratch_elems = 0;       // the sum of the steps' writes
    bool invalid = false;
};

static inline mle_route make_mle_route(const mle_call& c)
{
    mle_route r;
    const size_t es = c.elem_bytes;
    if ((es != 4 && es != 8 && es != 16 && es != 32) || c.lg_n > MLE_MAX_LG || c.op < MLE_OP_FOLD || c.op > MLE_OP_ROUND
        || ((c.op == MLE_OP_FOLD || c.op == MLE_OP_ROUND) && c.lg_n == 0) || (c.op == MLE_OP_ROUND && (c.rows < 2 || c.rows > 5))) {
        r.invalid = true; return r;
    }
    const unsigned T = mle_tile_lg(es), lgN = c.lg_n;
    const size_t cap = (size_t)std::max(c.cus, 1u) * MLE_WG_PER_CU, pack = mle_pack(es);
    auto push = [&](mle_kernel k, unsigned tile_lg, unsigned vars, unsigned var_base, size_t tiles, size_t writes, bool vec) {
        mle_step s = mle_step();
        s.kernel = k; s.block = MLE_NT; s.tile_lg = tile_lg; s.vars = vars; s.var_base = var_base; s.tiles = tiles; s.writes = writes;
        s.grid = (unsigned)std::min(std::max<size_t>(tiles, 1), cap);
        s.vec = vec;
        r.steps[r.nsteps++] = s;
        r.scratch_elems += writes;
    };
    if (c.op == MLE_OP_FOLD || c.op == MLE_OP_ROUND) {
        // whole 16-byte accesses of pairs: n / 2 results (fold) or pairs (round) are at least one access
        const size_t half = (size_t)1 << (lgN - 1);
        const bool vec = es >= 16 || (c.aligned16 && half >= pack);
        const size_t tiles = lgN <= T ? 1 : (size_t)1 << (lgN - T);
        if (c.op == MLE_OP_FOLD) { push(MK_FOLD, T, 1, 0, tiles, 0, vec); return r; }
        push(MK_ROUND, T, 0, 0, tiles, 0, vec);
        r.steps[0].writes = (size_t)r.steps[0].grid * c.rows; r.scratch_elems = r.steps[0].writes;
        push(MK_ROUND_SUM, 0, 0, 0, r.steps[0].grid, c.rows, false);
        r.steps[1].grid = 1;
        return r;
    }
    if (c.op == MLE_OP_EQ) {
        const unsigned tl = std::min(lgN, T);
        push(MK_EQ, tl, lgN, 0, (size_t)1 << (lgN - tl), 0, es >= 16 || (c.aligned16 && tl == T));
        return r;
    }
    // evaluate: whole tiles first (the first pass reads the caller's table, the later ones the scratch, which is aligned)
    unsigned done = 0;
    while (done < lgN) {
        const unsigned tl = std::min(lgN - done, T);
        const size_t tiles = (size_t)1 << (lgN - done - tl);
        if (r.nsteps >= mle_route::CAP) { r.invalid = true; return r; }
        push(MK_BIND, tl, tl, done, tiles, tiles, es >= 16 || (tl == T && (done ? true : c.aligned16)));
        done += tl;
    }
    return r;
}

} // namespace sppark_amd
