// HOST EMULATION TEST HARNESS for the Merkle kernels (tests only; see emu_ntt.cpp).
// Runs the bodies of sppark_amd/csrc/merkle/merkle_kernels.hpp for every (work-group, lane) the GPU grid would cover, over
// the steps of the driver's own route (merkle_route.hpp make_merkle_route): no decision is made here.  The top kernel's
// barrier between two levels is the end of a loop over the lanes here, its two LDS buffers two arrays.
//
// The kernels do not know the field, only the words per element: ONE shared library serves tests/test_emulation_merkle.py
// and tests/test_merkle_route.py, and with -DEMU_MERKLE_MAIN the file is a stand-alone program that checks itself against
// known digests and against itself across layouts and element sizes (for a sanitizer run).
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/merkle/merkle_kernels.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace sppark_amd;

static merkle_route route_of(unsigned ew, unsigned lg_n, size_t width, int layout, int hash, unsigned cus)
{
    merkle_call c;
    c.elem_bytes = ew * 4; c.lg_n = lg_n; c.width = width; c.layout = layout; c.hash = hash; c.cus = cus;
    return make_merkle_route(c);
}

// ---- the route as integers (tests/test_merkle_route.py) ----
// call: {elem_bytes, lg_n, width, layout, hash, cus}
// out: {nsteps, invalid}, then per step {kernel, grid, block, first, lo, hi, fused, items}
extern "C" unsigned emu_merkle_route(const uint64_t call[6], uint64_t* out, unsigned cap)
{
    merkle_call c;
    c.elem_bytes = (size_t)call[0]; c.lg_n = (unsigned)call[1]; c.width = (size_t)call[2]; c.layout = (int)call[3]; c.hash = (int)call[4];
    c.cus = (unsigned)call[5];
    const merkle_route r = make_merkle_route(c);
    if (cap < 2 + 8 * r.nsteps) return 0;
    uint64_t* o = out;
    *o++ = r.nsteps; *o++ = r.invalid;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const merkle_step& s = r.steps[i];
        const uint64_t v[8] = {s.kernel, s.grid, s.block, s.first, s.lo, s.hi, s.fused, s.items};
        for (uint64_t x : v) *o++ = x;
    }
    return (unsigned)(o - out);
}
extern "C" unsigned emu_merkle_top() { return MERKLE_TOP; }
extern "C" unsigned emu_merkle_fused() { return MERKLE_S; }

template<unsigned EW, int HASH>
static void leaves_run(const merkle_step& s, mk_digest* tree, const void* in, size_t n, size_t width, size_t cs, size_t ls, int layout)
{
    for (unsigned b = 0; b < s.grid; b++)
        for (unsigned t = 0; t < s.block; t++) {
            if (layout == MERKLE_COLUMNS) merkle_leaf_lane<EW, HASH, true>(tree, in, n, width, cs, ls, b, s.grid, t);
            else                          merkle_leaf_lane<EW, HASH, false>(tree, in, n, width, cs, ls, b, s.grid, t);
        }
}

template<int HASH>
static void top_run(mk_digest* tree, mk_digest* root, unsigned lg_n, unsigned first)
{
    std::vector<mk_digest> even(MERKLE_TOP / 2), odd(MERKLE_TOP / 4);
    const mk_digest* src = tree + merkle_layer_offset(lg_n, first);
    for (unsigned l = first; l < lg_n; l++) {
        mk_digest* keep = ((l - first) & 1) ? odd.data() : even.data();
        for (unsigned t = 0; t < MERKLE_NT; t++)
            merkle_top_level<HASH>(tree + merkle_layer_offset(lg_n, l + 1), keep, src, (size_t)1 << (lg_n - l - 1), t);
        src = keep;
    }
    if (root != nullptr) *root = *src;
}

template<unsigned EW, int HASH>
static int commit_run(mk_digest* tree, mk_digest* root, const void* in, unsigned lg_n, size_t width, size_t cs, size_t ls, int layout, unsigned cus)
{
    const merkle_route rt = route_of(EW, lg_n, width, layout, HASH, cus);
    if (rt.invalid || rt.nsteps < 2) return -1;
    for (unsigned i = 0; i < rt.nsteps; i++) {
        const merkle_step& s = rt.steps[i];
        if (s.block != MERKLE_NT) return -1;
        if (s.kernel == MKK_LEAVES) leaves_run<EW, HASH>(s, tree, in, (size_t)1 << lg_n, width, cs, ls, layout);
        else if (s.kernel == MKK_NODES) {
            if (s.fused != MERKLE_S || s.lo != s.first + 1) return -1;
            for (unsigned b = 0; b < s.grid; b++)
                for (unsigned t = 0; t < s.block; t++) merkle_nodes_lane<HASH, MERKLE_S>(tree, lg_n, s.first, s.items, b, s.grid, t);
        } else {
            if (s.grid != 1 || s.items > MERKLE_TOP) return -1;
            top_run<HASH>(tree, root, lg_n, s.first);
        }
    }
    return 0;
}

// tree: 16-byte aligned, (2^(lg_n+1) - 1) * 32 bytes; root: 16-byte aligned or NULL; in: aligned to the element (16 at most)
extern "C" int emu_merkle_commit(void* tree, void* root, const void* in, unsigned ew, unsigned lg_n, size_t width, size_t col_stride,
                                 size_t leaf_stride, int hash, unsigned cus)
{
    const int layout = leaf_stride == 1 && col_stride >= ((size_t)1 << lg_n) ? MERKLE_COLUMNS : MERKLE_ROWS;
    if (layout == MERKLE_ROWS && !(col_stride == 1 && leaf_stride >= width)) return -2;
    if (((uintptr_t)tree | (uintptr_t)root) & 15 || (uintptr_t)in % (ew * 4 < 16 ? ew * 4 : 16)) return -3;
    mk_digest* tr = (mk_digest*)tree;
    mk_digest* rt = (mk_digest*)root;
#define EMU_GO(EW)                                                                                                          \
    return hash == MERKLE_BLAKE2S ? commit_run<EW, MERKLE_BLAKE2S>(tr, rt, in, lg_n, width, col_stride, leaf_stride, layout, cus) \
         : hash == MERKLE_SHA256  ? commit_run<EW, MERKLE_SHA256>(tr, rt, in, lg_n, width, col_stride, leaf_stride, layout, cus) : -4;
    switch (ew) {
        case 1: EMU_GO(1)
        case 2: EMU_GO(2)
        case 4: EMU_GO(4)
        case 8: EMU_GO(8)
    }
#undef EMU_GO
    return -5;
}

extern "C" int emu_merkle_open(void* paths, const void* tree, unsigned lg_n, const uint64_t* indices, size_t nidx)
{
    const size_t pieces = nidx * lg_n * 2;
    for (size_t g = 0; g < pieces; g++) merkle_open_item((mk_q*)paths, (const mk_q*)tree, lg_n, indices, g);
    return 0;
}

extern "C" int emu_merkle_gather(void* rows, const void* in, unsigned ew, size_t width, size_t col_stride, size_t leaf_stride,
                                 const uint64_t* indices, size_t nidx)
{
    const size_t nwords = nidx * width * ew;
    for (size_t g = 0; g < nwords; g++) merkle_gather_item((u32*)rows, (const u32*)in, width, col_stride, leaf_stride, ew, indices, g);
    return 0;
}

#ifdef EMU_MERKLE_MAIN
// Stand-alone self-check.  Known digests (Python's hashlib) of the messages m[i] = 7 i + 1 mod 256 of 4, 56, 64 and 132
// bytes; then, for every element size, both layouts with padded strides and lg_n 0 .. 16: the columns and the rows tree are
// the same bytes, the tree of EW-word elements equals the tree of the same bytes as 1-word elements, every node is the leaf
// digest of its children's 64 bytes, and paths and rows are the gathers' definitions.
struct kat { unsigned len; unsigned char want[2][32]; };
static const kat KATS[] = {
    {4, {{0x26,0x1f,0x31,0x9a,0x82,0xab,0x78,0x35,0x13,0xb8,0x45,0xb4,0x3b,0xdd,0xf3,0x75,0x2a,0xb6,0x32,0xb1,0x85,0xce,0x61,0xc1,0x7f,0xac,0xdc,0x6e,0xde,0xa8,0x27,0xfe},
         {0xf4,0xc9,0x67,0x0a,0x5c,0x59,0xe0,0x0b,0x89,0xd9,0xdd,0x11,0xdb,0x51,0x49,0x03,0xa3,0x3c,0xd1,0xdc,0xc6,0x59,0x8a,0x0c,0xfb,0x34,0xa5,0x6f,0x70,0x8c,0x9b,0x8f}}},
    {56, {{0x6e,0x67,0x7c,0x38,0xdb,0xe4,0xdf,0x67,0x1f,0xd2,0xf9,0xdb,0xf6,0xb6,0xc8,0xe1,0x50,0x63,0x31,0xc5,0xfa,0xea,0x7f,0x9a,0x52,0x27,0x9a,0x85,0xf3,0xca,0xbb,0x9b},
          {0xc3,0x7b,0x44,0xe5,0xf1,0xb1,0x85,0x54,0xb3,0x69,0x66,0xf4,0xf8,0xe0,0x8b,0xfb,0xf3,0x16,0x4c,0x4b,0x6c,0x10,0x37,0x4d,0x12,0xd8,0x98,0x50,0x89,0x20,0x73,0xc5}}},
    {64, {{0x1a,0xa2,0xab,0xc4,0x87,0x84,0xc4,0xb7,0xb5,0x09,0xe5,0x65,0x40,0xcc,0xde,0x67,0x29,0x03,0xc6,0x13,0xc7,0xaa,0x32,0xc1,0x39,0x6e,0x10,0xd7,0x16,0x35,0x1d,0xfe},
          {0x66,0xbd,0x46,0x33,0xed,0x6f,0x71,0xc4,0xec,0xfa,0x47,0x63,0xbf,0x7b,0xa1,0xc8,0xec,0x76,0x12,0xde,0x9a,0xa6,0xc0,0x57,0x8a,0x7b,0x67,0x52,0x07,0xc7,0x1e,0x0b}}},
    {132, {{0x58,0xa4,0x73,0x6c,0xaf,0x65,0x3e,0xa3,0x7c,0x96,0x54,0x30,0xd1,0xc0,0x72,0xfa,0x97,0x9f,0x7b,0x82,0x18,0x6a,0xb0,0x09,0x8c,0x23,0x5d,0xed,0x7f,0xed,0xc2,0xf3},
           {0xdb,0x41,0x15,0x53,0x80,0xe3,0x3e,0x7b,0xaa,0x65,0x0f,0x4b,0xba,0x92,0xfb,0xab,0xe6,0x62,0x22,0x96,0xbd,0xb6,0x3d,0xf7,0xc7,0x83,0x60,0xbc,0x88,0x48,0x81,0x1a}}},
};
static uint64_t g_seed = 0x9e3779b97f4a7c15ULL;
static uint64_t next64() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }
typedef std::vector<mk_q> buffer;                               // (16-byte aligned storage)
static buffer bytes_of(size_t n) { return buffer((n + 15) / 16 + 1); }

int main()
{
    const unsigned cus = 2;
    int bad = 0;
    for (const kat& k : KATS)
        for (int hash = 0; hash < 2; hash++) {
            buffer msg = bytes_of(k.len), tree = bytes_of(32);
            for (unsigned i = 0; i < k.len; i++) ((unsigned char*)msg.data())[i] = (unsigned char)(7 * i + 1);
            if (emu_merkle_commit(tree.data(), nullptr, msg.data(), 1, 0, k.len / 4, 1, 1, hash, cus)) bad++;
            if (memcmp(tree.data(), k.want[hash], 32)) { bad++; printf("known digest of %u bytes, hash %d: mismatch\n", k.len, hash); }
        }
    const size_t widths[] = {1, 2, 3, 5, 13, 16, 17, 33};
    for (unsigned ew = 1; ew <= 8; ew *= 2)
        for (unsigned lg = 0; lg <= 16; lg += (lg >= 12 && ew > 1 ? 4 : 1))
            for (size_t width : widths) {
                if (lg > 11 && width > 3) continue;
                const size_t n = (size_t)1 << lg, cs = n + 3, ls = width + 2, eb = ew * 4, tb = (2 * n - 1) * 32;
                buffer cols = bytes_of(width * cs * eb), rows = bytes_of(n * ls * eb), flat = bytes_of(n * width * eb);
                for (auto& q : cols) for (u32& w : q.w) w = (u32)next64();
                for (auto& q : rows) for (u32& w : q.w) w = (u32)next64();
                for (size_t i = 0; i < n; i++)
                    for (size_t j = 0; j < width; j++) {
                        memcpy((char*)rows.data() + (i * ls + j) * eb, (char*)cols.data() + (j * cs + i) * eb, eb);
                        memcpy((char*)flat.data() + (i * width + j) * eb, (char*)cols.data() + (j * cs + i) * eb, eb);
                    }
                for (int hash = 0; hash < 2; hash++) {
                    buffer t1 = bytes_of(tb), t2 = bytes_of(tb), t3 = bytes_of(tb), root = bytes_of(32);
                    if (emu_merkle_commit(t1.data(), root.data(), cols.data(), ew, lg, width, cs, 1, hash, cus)) bad++;
                    if (emu_merkle_commit(t2.data(), nullptr, rows.data(), ew, lg, width, 1, ls, hash, cus)) bad++;
                    if (emu_merkle_commit(t3.data(), nullptr, flat.data(), 1, lg, width * ew, 1, width * ew, hash, cus)) bad++;
                    if (memcmp(t1.data(), t2.data(), tb) || memcmp(t1.data(), t3.data(), tb)) { bad++; printf("ew %u lg %u width %zu hash %d: trees differ\n", ew, lg, width, hash); }
                    if (memcmp(root.data(), (char*)t1.data() + tb - 32, 32)) bad++;
                    // every node is the digest of its children's 64 bytes: the tree over layer l as leaves of 16 words is layer l + 1
                    if (lg >= 1 && lg <= 11) {
                        for (unsigned l = 0; l < lg; l++) {
                            const size_t cnt = (size_t)1 << (lg - l - 1);
                            buffer up = bytes_of((2 * cnt - 1) * 32);
                            if (emu_merkle_commit(up.data(), nullptr, (char*)t1.data() + merkle_layer_offset(lg, l) * 32, 1, lg - l - 1, 16, 1, 16, hash, cus)) bad++;
                            if (memcmp(up.data(), (char*)t1.data() + merkle_layer_offset(lg, l + 1) * 32, cnt * 32)) { bad++; printf("lg %u layer %u: nodes differ\n", lg, l + 1); }
                        }
                    }
                    const uint64_t idx[3] = {0, n - 1, next64() & (n - 1)};
                    buffer paths = bytes_of(3 * (lg ? lg : 1) * 32), got = bytes_of(3 * width * eb);
                    emu_merkle_open(paths.data(), t1.data(), lg, idx, 3);
                    emu_merkle_gather(got.data(), cols.data(), ew, width, cs, 1, idx, 3);
                    for (unsigned q = 0; q < 3; q++) {
                        for (unsigned l = 0; l < lg; l++)
                            if (memcmp((char*)paths.data() + (q * lg + l) * 32, (char*)t1.data() + (merkle_layer_offset(lg, l) + ((idx[q] >> l) ^ 1)) * 32, 32)) bad++;
                        if (memcmp((char*)got.data() + q * width * eb, (char*)flat.data() + idx[q] * width * eb, width * eb)) bad++;
                    }
                }
            }
    printf("emu_merkle self-check, elements of 1 .. 8 words, lg_n 0 .. 16: %s (%d mismatches)\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
#endif
