// The launches of one Merkle commitment (include/sppark_amd_merkle.h), decided in ONE pure function: make_merkle_route(call)
// returns the steps as data -- kernel, grid, the layer a step reads, the layers it writes.  No HIP calls;
// api/merkle_api.hpp launches what it returns and tests/emu/emu_merkle.cpp runs the same steps on the host.
//
// Layer l (0 = leaf digests .. lg_n = root) holds 2^(lg_n - l) digests of 32 bytes.
//
//   leaves  one launch: a lane hashes one leaf of the matrix into layer 0; a work-group takes tiles of MERKLE_NT consecutive
//           leaves and strides over them by the grid.  Nothing of the tree is folded into this kernel: a lane that hashed
//           two leaves and their parent would halve the coalesced width of a wave's load for one saved pass over 64 bytes
//           per leaf pair, and no measurement has favoured it ("Merkle commitments").
//   nodes   while a layer holds more than MERKLE_TOP digests: a lane reads 2^MERKLE_S consecutive digests of layer |first|
//           and writes layers first + 1 .. first + MERKLE_S; no LDS, no barrier.
//   top     one work-group takes the first layer of at most MERKLE_TOP digests to the root through LDS, and copies the
//           root out.  MERKLE_TOP = 1024: the 512 + 256 digests the two LDS buffers hold are 24 KiB of the CU's 160 KiB, and
//           the longest chain of one lane is 2 + 1 + 8 compressions; twice the size would double that chain on ONE CU
//           for the sake of a launch that the nodes kernel spreads over four work-groups.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sppark_amd {

enum { MERKLE_BLAKE2S = 0, MERKLE_SHA256 = 1 };
enum { MERKLE_COLUMNS = 0, MERKLE_ROWS = 1 };
enum merkle_kernel : unsigned char { MKK_LEAVES, MKK_NODES, MKK_TOP };

static constexpr unsigned MERKLE_NT = 256;              // lanes per work-group
static constexpr unsigned MERKLE_WG_PER_CU = 8;         // the grid's cap: work-groups per CU
static constexpr unsigned MERKLE_MAX_LG = 28;
static constexpr unsigned MERKLE_S = 3;                 // layers per nodes launch
static constexpr unsigned MERKLE_TOP = 1024;            // digests of the layer the top kernel starts from, at most
static constexpr unsigned MERKLE_TOP_LG = 10;

// digest index of the first digest of layer l
static inline constexpr size_t merkle_layer_offset(unsigned lg_n, unsigned l)
{   return ((size_t)2 << lg_n) - ((size_t)2 << (lg_n - l));   }

struct merkle_call {
    size_t elem_bytes = 8;
    unsigned lg_n = 0;
    size_t width = 1;
    int layout = MERKLE_COLUMNS;
    int hash = MERKLE_BLAKE2S;
    unsigned cus = 1;
};

struct merkle_step {
    merkle_kernel kernel;
    unsigned grid, block;
    unsigned first;                 // the layer the step reads (leaves: none, it reads the matrix)
    unsigned lo, hi;                // the layers it writes: lo .. hi (top at lg_n <= 0 layers above |first|: lo > hi, none)
    unsigned fused;                 // hi - lo + 1
    size_t items;                   // leaves: leaves; nodes: lanes' subtrees; top: digests of layer |first|
};

struct merkle_route {
    static constexpr unsigned CAP = 12;
    merkle_step steps[CAP];
    unsigned nsteps = 0;
    bool invalid = false;
};

static inline merkle_route make_merkle_route(const merkle_call& c)
{
    merkle_route r;
    const size_t es = c.elem_bytes;
    if ((es != 4 && es != 8 && es != 16 && es != 32) || c.lg_n > MERKLE_MAX_LG || c.width == 0 || c.width > (size_t)0xffffffffu / es
        || (c.layout != MERKLE_COLUMNS && c.layout != MERKLE_ROWS) || (c.hash != MERKLE_BLAKE2S && c.hash != MERKLE_SHA256)) {
        r.invalid = true; return r;
    }
    const size_t cap = (size_t)std::max(c.cus, 1u) * MERKLE_WG_PER_CU;
    auto push = [&](merkle_kernel k, unsigned first, unsigned lo, unsigned hi, size_t items, size_t groups) {
        merkle_step s = merkle_step();
        s.kernel = k; s.block = MERKLE_NT; s.first = first; s.lo = lo; s.hi = hi; s.fused = hi + 1 - lo; s.items = items;
        s.grid = (unsigned)std::min(std::max<size_t>(groups, 1), cap);
        r.steps[r.nsteps++] = s;
    };
    const size_t n = (size_t)1 << c.lg_n;
    push(MKK_LEAVES, 0, 0, 0, n, (n + MERKLE_NT - 1) / MERKLE_NT);
    unsigned l = 0;
    while (c.lg_n - l > MERKLE_TOP_LG) {
        const size_t lanes = (size_t)1 << (c.lg_n - l - MERKLE_S);
        push(MKK_NODES, l, l + 1, l + MERKLE_S, lanes, (lanes + MERKLE_NT - 1) / MERKLE_NT);
        l += MERKLE_S;
    }
    push(MKK_TOP, l, l + 1, c.lg_n, (size_t)1 << (c.lg_n - l), 1);
    return r;
}

} // namespace sppark_amd
