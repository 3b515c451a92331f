// The launches of one Poseidon2 call (include/sppark_amd_poseidon2.h), decided in ONE pure function:
// make_poseidon2_route(call) returns the steps as data -- kernel, grid, the layer a step reads, the layers it writes.  No HIP
// calls; api/poseidon2_api.hpp launches what it returns and tests/emu/emu_poseidon2.cpp runs the same steps on the host.
//
// The tree is the tree of merkle/merkle_route.hpp (its layer offsets are used as they are): layer l (0 = leaf digests ..
// lg_n = root) holds 2^(lg_n - l) digests of 32 bytes = T / 2 field elements.
//
//   permute one launch: a lane permutes one state of T elements; a work-group strides over tiles of P2_NT states by the grid.
//   leaves  one launch: a lane absorbs one leaf of the matrix (ceil(width / RATE) permutations) into layer 0.
//   nodes   while a layer holds more than P2_TOP digests: a lane reads 2^P2_S consecutive digests of layer |first| and
//           writes layers first + 1 .. first + P2_S; no LDS, no barrier.  P2_S = 3: the eight digests are 64 registers in
//           both fields (8 x 8 words of BabyBear, 8 x 4 double words of Goldilocks) next to the 16 of the state and the
//           products' temporaries: the kernel takes 76 (BabyBear) and 81 (Goldilocks) registers, inside the 128 at which a
//           SIMD still holds four waves (tests/test_poseidon2_abi.py asserts it); S = 4 would need 128 for the digests alone.
//           Seven permutations per lane and launch, every lane busy at every level.
//   top     one work-group takes the first layer of at most P2_TOP = 1024 digests to the root through LDS (512 + 256
//           digests, 24 KiB) and copies the root out: the geometry of the byte-hash trees, for their reasons.
#pragma once
#include "../merkle/merkle_route.hpp"

namespace sppark_amd {

enum p2_kernel : unsigned char { P2K_PERMUTE, P2K_LEAVES, P2K_NODES, P2K_TOP };
enum { P2_OP_PERMUTE = 0, P2_OP_COMMIT = 1 };

static constexpr unsigned P2_NT = 256;                  // lanes per work-group
static constexpr unsigned P2_WG_PER_CU = 8;             // the grid's cap: work-groups per CU
static constexpr unsigned P2_MAX_LG = MERKLE_MAX_LG;
static constexpr unsigned P2_S = 3;                     // layers per nodes launch
static constexpr unsigned P2_TOP = 1024;                // digests of the layer the top kernel starts from, at most
static constexpr unsigned P2_TOP_LG = 10;
static constexpr unsigned P2_MAX_RF = 16, P2_MAX_RP = 64;

// elements of a state for an element of |elem_bytes| bytes: 16 words of BabyBear, 8 double words of Goldilocks (64 bytes)
static inline constexpr unsigned p2_width_of(size_t elem_bytes) { return elem_bytes == 4 ? 16 : elem_bytes == 8 ? 8 : 0; }
// elements of the constants buffer: external constants round by round, internal constants, the diagonal
static inline constexpr size_t p2_const_count(unsigned t, unsigned rounds_f, unsigned rounds_p)
{   return (size_t)rounds_f * t + rounds_p + t;   }
static inline constexpr bool p2_rounds_ok(unsigned rounds_f, unsigned rounds_p)
{   return rounds_f >= 2 && rounds_f <= P2_MAX_RF && (rounds_f & 1) == 0 && rounds_p <= P2_MAX_RP;   }

struct p2_call {
    int op = P2_OP_COMMIT;
    size_t elem_bytes = 4;
    unsigned rounds_f = 8, rounds_p = 13;
    size_t count = 0;               // permute: states
    unsigned lg_n = 0;              // commit
    size_t width = 1;
    int layout = MERKLE_COLUMNS;
    unsigned cus = 1;
};

struct p2_step {
    p2_kernel kernel;
    unsigned grid, block;
    unsigned first;                 // the layer the step reads (permute, leaves: none)
    unsigned lo, hi;                // the layers it writes: lo .. hi (top over a single digest: lo > hi, none)
    unsigned fused;                 // hi - lo + 1
    size_t items;                   // permute: states; leaves: leaves; nodes: lanes' subtrees; top: digests of layer |first|
};

struct p2_route {
    static constexpr unsigned CAP = 12;
    p2_step steps[CAP];
    unsigned nsteps = 0;
    bool invalid = false;
};

static inline p2_route make_poseidon2_route(const p2_call& c)
{
    p2_route r;
    const unsigned t = p2_width_of(c.elem_bytes);
    if (t == 0 || !p2_rounds_ok(c.rounds_f, c.rounds_p) || (c.op != P2_OP_PERMUTE && c.op != P2_OP_COMMIT)) { r.invalid = true; return r; }
    const size_t cap = (size_t)std::max(c.cus, 1u) * P2_WG_PER_CU;
    auto push = [&](p2_kernel k, unsigned first, unsigned lo, unsigned hi, size_t items, size_t groups) {
        p2_step s = p2_step();
        s.kernel = k; s.block = P2_NT; s.first = first; s.lo = lo; s.hi = hi; s.fused = hi + 1 - lo; s.items = items;
        s.grid = (unsigned)std::min(std::max<size_t>(groups, 1), cap);
        r.steps[r.nsteps++] = s;
    };
    if (c.op == P2_OP_PERMUTE) {
        if (c.count == 0 || c.count > ((size_t)-1) / 64) { r.invalid = true; return r; }
        push(P2K_PERMUTE, 0, 1, 0, c.count, (c.count + P2_NT - 1) / P2_NT);
        return r;
    }
    if (c.lg_n > P2_MAX_LG || c.width == 0 || c.width > (size_t)0xffffffffu / c.elem_bytes
        || (c.layout != MERKLE_COLUMNS && c.layout != MERKLE_ROWS)) {
        r.invalid = true; return r;
    }
    const size_t n = (size_t)1 << c.lg_n;
    push(P2K_LEAVES, 0, 0, 0, n, (n + P2_NT - 1) / P2_NT);
    unsigned l = 0;
    while (c.lg_n - l > P2_TOP_LG) {
        const size_t lanes = (size_t)1 << (c.lg_n - l - P2_S);
        push(P2K_NODES, l, l + 1, l + P2_S, lanes, (lanes + P2_NT - 1) / P2_NT);
        l += P2_S;
    }
    push(P2K_TOP, l, l + 1, c.lg_n, (size_t)1 << (c.lg_n - l), 1);
    return r;
}

} // namespace sppark_amd
