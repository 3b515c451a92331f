// Merkle commitments (include/sppark_amd_merkle.h): leaf digests of a matrix of field elements, the binary tree above them,
// authentication paths and opened rows.  The reference's snapshot has no counterpart (its README names hash/ and merkle/).
//
// The hashes are unkeyed BLAKE2s-256 (RFC 7693) and SHA-256 (FIPS 180-4): 32-bit add / xor / rotate code, bound by
// instruction issue, without a multiplier and -- outside the top kernel -- without LDS.  The elements are opaque bytes: the
// kernels are templated on the 32-bit words per element EW (1, 2, 4, 8) and on the hash, not on a field class.
//
// The 16 message words and the 8 chaining / 16 working words live in registers only as long as every index into them is a
// compile-time constant: the rounds below are written out with literal indices (MK_B2S_ROUND, MK_SHA_R), and every loop
// that fills or copies such an array has a constant trip count and is unrolled.  tests/test_merkle_abi.py reads the code
// objects' metadata: no kernel here has a private segment.
//
// Geometry (merkle_route.hpp): MERKLE_NT lanes; a work-group strides over its items in steps of the grid.
//
//   k_merkle_leaves<EW, HASH, COLUMNS>  one leaf per lane.  Element j of leaf i lies at (j * col_stride + i * leaf_stride)
//                       elements: in the columns layout (leaf_stride == 1) the 64 lanes of a wave read 64 * EW * 4
//                       contiguous bytes per element, in the rows layout (col_stride == 1) a lane walks its own row.  EW
//                       divides 16, so a 64-byte block is 16 / EW whole elements; a load past |width| is predicated to zero.
//                       BLAKE2s: the last block carries the byte count and the final flag (no empty block after a leaf of
//                       a multiple of 64 bytes).  SHA-256: words are byte-swapped at load; 0x80 lands in a whole word as
//                       leaves are multiples of 4 bytes; a block of padding alone follows when leaf_bytes mod 64 > 52.
//   k_merkle_nodes<HASH, S>  a lane reads 2^S consecutive digests of one layer (S = 3: 256 contiguous bytes, 16 dwordx4
//                       loads), hashes them down to one and writes every layer between: S layers per launch, every lane
//                       busy at every level.  SHA-256's second block of a 64-byte message is constant padding; its
//                       schedule folds into constants at compile time (mk_sha256_pad64).
//   k_merkle_top<HASH>  one work-group takes a layer of at most MERKLE_TOP digests to the root, level by level through two
//                       LDS buffers, writes every layer into the tree as well and the root to |root| if given.
//   k_merkle_open / k_merkle_gather  plain gathers: 16 bytes of a digest / one word of an element per lane.
//
// All offsets are 64-bit: the tree crosses 4 GiB at lg_n = 27, the matrix much earlier.
//
// The *_lane / *_level / *_item functions are the kernels' bodies; tests/emu/emu_merkle.cpp runs them on the host for every
// (work-group, lane) of the route's grids (the kernels themselves are left out of that build: it links without a device image).
#pragma once
#include "../ff/mont_dev.hpp"
#include "merkle_route.hpp"

namespace sppark_amd {

struct alignas(16) mk_digest { u32 w[8]; };                                 // 32 bytes, moved as two 16-byte accesses
struct alignas(16) mk_q { u32 w[4]; };
template<unsigned EW> struct alignas(EW * 4 >= 16 ? 16 : EW * 4) mk_elem { u32 w[EW]; };

SPPARK_DEVFN u32 mk_rotr(u32 x, unsigned n) { return (x >> n) | (x << (32 - n)); }
SPPARK_DEVFN u32 mk_bswap(u32 x) { return __builtin_bswap32(x); }

// ---- BLAKE2s (RFC 7693, section 3) ----------------------------------------------------------------------------------------
#define MK_B2S_G(a, b, c, d, x, y)                                                                                          \
    a = a + b + (x); d = mk_rotr(d ^ a, 16); c = c + d; b = mk_rotr(b ^ c, 12);                                             \
    a = a + b + (y); d = mk_rotr(d ^ a, 8);  c = c + d; b = mk_rotr(b ^ c, 7);
#define MK_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                                  \
    MK_B2S_G(v0, v4, v8,  v12, m[s0],  m[s1])  MK_B2S_G(v1, v5, v9,  v13, m[s2],  m[s3])                                    \
    MK_B2S_G(v2, v6, v10, v14, m[s4],  m[s5])  MK_B2S_G(v3, v7, v11, v15, m[s6],  m[s7])                                    \
    MK_B2S_G(v0, v5, v10, v15, m[s8],  m[s9])  MK_B2S_G(v1, v6, v11, v12, m[s10], m[s11])                                   \
    MK_B2S_G(v2, v7, v8,  v13, m[s12], m[s13]) MK_B2S_G(v3, v4, v9,  v14, m[s14], m[s15])

// h: the chaining value; m: 16 little-endian message words; t: bytes hashed up to and including this block (< 2^32)
SPPARK_DEVFN void mk_blake2s_compress(u32 (&h)[8], const u32 (&m)[16], u32 t, bool last)
{
    u32 v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
    u32 v8 = 0x6a09e667u, v9 = 0xbb67ae85u, v10 = 0x3c6ef372u, v11 = 0xa54ff53au;
    u32 v12 = 0x510e527fu ^ t, v13 = 0x9b05688cu, v14 = last ? ~0x1f83d9abu : 0x1f83d9abu, v15 = 0x5be0cd19u;
    MK_B2S_ROUND( 0,  1,  2,  3,  4,  5,  6,  7,  8,  9, 10, 11, 12, 13, 14, 15)
    MK_B2S_ROUND(14, 10,  4,  8,  9, 15, 13,  6,  1, 12,  0,  2, 11,  7,  5,  3)
    MK_B2S_ROUND(11,  8, 12,  0,  5,  2, 15, 13, 10, 14,  3,  6,  7,  1,  9,  4)
    MK_B2S_ROUND( 7,  9,  3,  1, 13, 12, 11, 14,  2,  6,  5, 10,  4,  0, 15,  8)
    MK_B2S_ROUND( 9,  0,  5,  7,  2,  4, 10, 15, 14,  1, 11, 12,  6,  8,  3, 13)
    MK_B2S_ROUND( 2, 12,  6, 10,  0, 11,  8,  3,  4, 13,  7,  5, 15, 14,  1,  9)
    MK_B2S_ROUND(12,  5,  1, 15, 14, 13,  4, 10,  0,  7,  6,  3,  9,  2,  8, 11)
    MK_B2S_ROUND(13, 11,  7, 14, 12,  1,  3,  9,  5,  0, 15,  4,  8,  6,  2, 10)
    MK_B2S_ROUND( 6, 15, 14,  9, 11,  3,  0,  8, 12,  2, 13,  7,  1,  4, 10,  5)
    MK_B2S_ROUND(10,  2,  8,  4,  7,  6,  1,  5, 15, 11,  9, 14,  3, 12, 13,  0)
    h[0] ^= v0 ^ v8;  h[1] ^= v1 ^ v9;  h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11;
    h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

// ---- SHA-256 (FIPS 180-4, section 6.2) ------------------------------------------------------------------------------------
// round t with the schedule kept in 16 words: w[t & 15] is W_t
#define MK_SHA_R(t, K)                                                                                                      \
    {                                                                                                                       \
        if ((t) >= 16) {                                                                                                    \
            const u32 x = w[((t) + 1) & 15], y = w[((t) + 14) & 15];                                                        \
            w[(t) & 15] += (mk_rotr(x, 7) ^ mk_rotr(x, 18) ^ (x >> 3)) + w[((t) + 9) & 15]                                  \
                         + (mk_rotr(y, 17) ^ mk_rotr(y, 19) ^ (y >> 10));                                                   \
        }                                                                                                                   \
        const u32 t1 = hh + (mk_rotr(e, 6) ^ mk_rotr(e, 11) ^ mk_rotr(e, 25)) + ((e & f) ^ (~e & g)) + (K) + w[(t) & 15];   \
        const u32 t2 = (mk_rotr(a, 2) ^ mk_rotr(a, 13) ^ mk_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));                   \
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;                                                 \
    }

// h: the hash value; m: 16 big-endian message words (as integers)
SPPARK_DEVFN void mk_sha256_compress(u32 (&h)[8], const u32 (&m)[16])
{
    u32 w[16];
    #pragma unroll
    for (unsigned i = 0; i < 16; i++) w[i] = m[i];
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    MK_SHA_R( 0, 0x428a2f98u) MK_SHA_R( 1, 0x71374491u) MK_SHA_R( 2, 0xb5c0fbcfu) MK_SHA_R( 3, 0xe9b5dba5u)
    MK_SHA_R( 4, 0x3956c25bu) MK_SHA_R( 5, 0x59f111f1u) MK_SHA_R( 6, 0x923f82a4u) MK_SHA_R( 7, 0xab1c5ed5u)
    MK_SHA_R( 8, 0xd807aa98u) MK_SHA_R( 9, 0x12835b01u) MK_SHA_R(10, 0x243185beu) MK_SHA_R(11, 0x550c7dc3u)
    MK_SHA_R(12, 0x72be5d74u) MK_SHA_R(13, 0x80deb1feu) MK_SHA_R(14, 0x9bdc06a7u) MK_SHA_R(15, 0xc19bf174u)
    MK_SHA_R(16, 0xe49b69c1u) MK_SHA_R(17, 0xefbe4786u) MK_SHA_R(18, 0x0fc19dc6u) MK_SHA_R(19, 0x240ca1ccu)
    MK_SHA_R(20, 0x2de92c6fu) MK_SHA_R(21, 0x4a7484aau) MK_SHA_R(22, 0x5cb0a9dcu) MK_SHA_R(23, 0x76f988dau)
    MK_SHA_R(24, 0x983e5152u) MK_SHA_R(25, 0xa831c66du) MK_SHA_R(26, 0xb00327c8u) MK_SHA_R(27, 0xbf597fc7u)
    MK_SHA_R(28, 0xc6e00bf3u) MK_SHA_R(29, 0xd5a79147u) MK_SHA_R(30, 0x06ca6351u) MK_SHA_R(31, 0x14292967u)
    MK_SHA_R(32, 0x27b70a85u) MK_SHA_R(33, 0x2e1b2138u) MK_SHA_R(34, 0x4d2c6dfcu) MK_SHA_R(35, 0x53380d13u)
    MK_SHA_R(36, 0x650a7354u) MK_SHA_R(37, 0x766a0abbu) MK_SHA_R(38, 0x81c2c92eu) MK_SHA_R(39, 0x92722c85u)
    MK_SHA_R(40, 0xa2bfe8a1u) MK_SHA_R(41, 0xa81a664bu) MK_SHA_R(42, 0xc24b8b70u) MK_SHA_R(43, 0xc76c51a3u)
    MK_SHA_R(44, 0xd192e819u) MK_SHA_R(45, 0xd6990624u) MK_SHA_R(46, 0xf40e3585u) MK_SHA_R(47, 0x106aa070u)
    MK_SHA_R(48, 0x19a4c116u) MK_SHA_R(49, 0x1e376c08u) MK_SHA_R(50, 0x2748774cu) MK_SHA_R(51, 0x34b0bcb5u)
    MK_SHA_R(52, 0x391c0cb3u) MK_SHA_R(53, 0x4ed8aa4au) MK_SHA_R(54, 0x5b9cca4fu) MK_SHA_R(55, 0x682e6ff3u)
    MK_SHA_R(56, 0x748f82eeu) MK_SHA_R(57, 0x78a5636fu) MK_SHA_R(58, 0x84c87814u) MK_SHA_R(59, 0x8cc70208u)
    MK_SHA_R(60, 0x90befffau) MK_SHA_R(61, 0xa4506cebu) MK_SHA_R(62, 0xbef9a3f7u) MK_SHA_R(63, 0xc67178f2u)
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// the block that follows a message of exactly 64 bytes: 0x80, zeros, the length 512; every word is a constant, so the
// schedule is too
SPPARK_DEVFN void mk_sha256_pad64(u32 (&h)[8])
{
    const u32 m[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512};
    mk_sha256_compress(h, m);
}

// ---- the two hashes behind one interface -----------------------------------------------------------------------------------
template<int HASH> struct mk_hash;

template<> struct mk_hash<MERKLE_BLAKE2S> {
    static SPPARK_DEVFN void init(u32 (&h)[8])
    {
        h[0] = 0x6a09e667u ^ 0x01010020u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;      // digest 32, no key, fanout = depth = 1
        h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
    }
    static SPPARK_DEVFN size_t blocks(u32 bytes) { return bytes <= 64 ? 1 : ((size_t)bytes + 63) / 64; }
    // block |b| of |nb| of a message of |words| words; m: the message words as stored, zero beyond the message
    static SPPARK_DEVFN void block(u32 (&h)[8], u32 (&m)[16], size_t b, size_t nb, size_t words)
    {
        const bool last = b + 1 == nb;
        mk_blake2s_compress(h, m, last ? (u32)(words * 4) : (u32)((b + 1) * 64), last);
    }
    static SPPARK_DEVFN void node(mk_digest& out, const mk_digest& l, const mk_digest& r)
    {
        u32 h[8], m[16];
        init(h);
        #pragma unroll
        for (unsigned i = 0; i < 8; i++) { m[i] = l.w[i]; m[8 + i] = r.w[i]; }
        mk_blake2s_compress(h, m, 64, true);
        #pragma unroll
        for (unsigned i = 0; i < 8; i++) out.w[i] = h[i];
    }
    static SPPARK_DEVFN void digest(mk_digest& out, const u32 (&h)[8])
    {
        #pragma unroll
        for (unsigned i = 0; i < 8; i++) out.w[i] = h[i];
    }
};

template<> struct mk_hash<MERKLE_SHA256> {
    static SPPARK_DEVFN void init(u32 (&h)[8])
    {
        h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
        h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
    }
    static SPPARK_DEVFN size_t blocks(u32 bytes) { return ((size_t)bytes + 9 + 63) / 64; }     // 0x80 and the 64-bit length
    static SPPARK_DEVFN void block(u32 (&h)[8], u32 (&m)[16], size_t b, size_t nb, size_t words)
    {
        #pragma unroll
        for (unsigned i = 0; i < 16; i++) {
            const size_t k = b * 16 + i;
            m[i] = k < words ? mk_bswap(m[i]) : k == words ? 0x80000000u : 0u;
        }
        if (b + 1 == nb) { m[14] = (u32)(words >> 27); m[15] = (u32)(words << 5); }             // the length in bits: words * 32
        mk_sha256_compress(h, m);
    }
    static SPPARK_DEVFN void node(mk_digest& out, const mk_digest& l, const mk_digest& r)
    {
        u32 h[8], m[16];
        init(h);
        #pragma unroll
        for (unsigned i = 0; i < 8; i++) { m[i] = mk_bswap(l.w[i]); m[8 + i] = mk_bswap(r.w[i]); }
        mk_sha256_compress(h, m);
        mk_sha256_pad64(h);
        digest(out, h);
    }
    static SPPARK_DEVFN void digest(mk_digest& out, const u32 (&h)[8])
    {
        #pragma unroll
        for (unsigned i = 0; i < 8; i++) out.w[i] = mk_bswap(h[i]);
    }
};

// ---- leaves -----------------------------------------------------------------------------------------------------------------
// the whole work of lane |t| of work-group |block| of |nblocks|: layer 0 of |tree|
template<unsigned EW, int HASH, bool COLUMNS>
SPPARK_DEVFN void merkle_leaf_lane(mk_digest* tree, const void* in, size_t n, size_t width, size_t col_stride, size_t leaf_stride,
                                   unsigned block, unsigned nblocks, unsigned t)
{
    typedef mk_elem<EW> elem;
    typedef mk_hash<HASH> H;
    constexpr unsigned PER = 16 / EW;                                       // elements of a 64-byte block
    const size_t words = width * EW;                                        // (< 2^30: the entry point's check)
    const size_t nb = H::blocks((u32)(words * 4));
    for (size_t i = (size_t)block * MERKLE_NT + t; i < n; i += (size_t)nblocks * MERKLE_NT) {
        const elem* p = reinterpret_cast<const elem*>(in) + (COLUMNS ? i : i * leaf_stride);
        u32 h[8];
        H::init(h);
        for (size_t b = 0; b < nb; b++) {
            u32 m[16];
            #pragma unroll
            for (unsigned e = 0; e < PER; e++) {
                const size_t j = b * PER + e;
                elem x;
                #pragma unroll
                for (unsigned k = 0; k < EW; k++) x.w[k] = 0;
                if (j < width) x = p[COLUMNS ? j * col_stride : j];
                #pragma unroll
                for (unsigned k = 0; k < EW; k++) m[e * EW + k] = x.w[k];
            }
            H::block(h, m, b, nb, words);
        }
        mk_digest dg;
        H::digest(dg, h);
        tree[i] = dg;
    }
}

#ifndef SPPARK_HOST_EMULATION
template<unsigned EW, int HASH, bool COLUMNS>
__global__ __launch_bounds__(MERKLE_NT)
void k_merkle_leaves(mk_digest* tree, const void* in, size_t n, size_t width, size_t col_stride, size_t leaf_stride)
{
#if defined(__HIP_DEVICE_COMPILE__)
    merkle_leaf_lane<EW, HASH, COLUMNS>(tree, in, n, width, col_stride, leaf_stride, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}
#endif

// ---- nodes: lane-local subtrees ------------------------------------------------------------------------------------------------
// node K of level LV of a lane's subtree, then the nodes after it and the levels above: level LV makes 2^(S - LV) digests
// from twice as many and writes them into layer first + LV.  One instance per node instead of loops: the SHA-256 body is
// too large for the compiler to unroll a loop around it, and a loop left standing indexes d[] at run time, which sends the
// eight digests to scratch.
template<int HASH, unsigned S, unsigned LV, unsigned K>
SPPARK_DEVFN void merkle_nodes_from(mk_digest (&d)[1u << S], mk_digest* tree, unsigned lg_n, unsigned first, size_t g)
{
    constexpr unsigned CNT = (1u << S) >> LV;
    mk_digest r;
    mk_hash<HASH>::node(r, d[2 * K], d[2 * K + 1]);
    d[K] = r;
    tree[merkle_layer_offset(lg_n, first + LV) + g * CNT + K] = r;
    if constexpr (K + 1 < CNT) merkle_nodes_from<HASH, S, LV, K + 1>(d, tree, lg_n, first, g);
    else if constexpr (LV < S) merkle_nodes_from<HASH, S, LV + 1, 0>(d, tree, lg_n, first, g);
}

// lane |t| of work-group |block|: subtrees g of the |lanes| of layer |first|, 2^S digests in, layers first + 1 .. first + S out
template<int HASH, unsigned S>
SPPARK_DEVFN void merkle_nodes_lane(mk_digest* tree, unsigned lg_n, unsigned first, size_t lanes, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned C = 1u << S;
    for (size_t g = (size_t)block * MERKLE_NT + t; g < lanes; g += (size_t)nblocks * MERKLE_NT) {
        mk_digest d[C];
        const mk_digest* src = tree + merkle_layer_offset(lg_n, first) + g * C;
        #pragma unroll
        for (unsigned k = 0; k < C; k++) d[k] = src[k];
        merkle_nodes_from<HASH, S, 1, 0>(d, tree, lg_n, first, g);
    }
}

#ifndef SPPARK_HOST_EMULATION
template<int HASH, unsigned S>
__global__ __launch_bounds__(MERKLE_NT)
void k_merkle_nodes(mk_digest* tree, unsigned lg_n, unsigned first, size_t lanes)
{
#if defined(__HIP_DEVICE_COMPILE__)
    merkle_nodes_lane<HASH, S>(tree, lg_n, first, lanes, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}
#endif

// ---- top: one work-group to the root ---------------------------------------------------------------------------------------
// one level for lane |t|: |parents| digests from the 2 * parents at |src|, kept at |keep| (LDS) and written to |out| (the tree)
template<int HASH>
SPPARK_DEVFN void merkle_top_level(mk_digest* out, mk_digest* keep, const mk_digest* src, size_t parents, unsigned t)
{
    for (size_t i = t; i < parents; i += MERKLE_NT) {
        mk_digest r;
        mk_hash<HASH>::node(r, src[2 * i], src[2 * i + 1]);
        keep[i] = r;
        out[i] = r;
    }
}

#ifndef SPPARK_HOST_EMULATION
template<int HASH>
__global__ __launch_bounds__(MERKLE_NT)
void k_merkle_top(mk_digest* tree, mk_digest* root, unsigned lg_n, unsigned first)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ mk_digest even[MERKLE_TOP / 2], odd[MERKLE_TOP / 4];         // the levels alternate between them
    const mk_digest* src = tree + merkle_layer_offset(lg_n, first);
    for (unsigned l = first; l < lg_n; l++) {
        mk_digest* keep = ((l - first) & 1) ? odd : even;
        merkle_top_level<HASH>(tree + merkle_layer_offset(lg_n, l + 1), keep, src, (size_t)1 << (lg_n - l - 1), threadIdx.x);
        __syncthreads();
        src = keep;
    }
    if (root != nullptr && threadIdx.x == 0) *root = *src;                  // (lg_n == first: the one digest of the layer)
#endif
}
#endif

// ---- open and gather ---------------------------------------------------------------------------------------------------------
// (both items are host functions too: a tree or a matrix on the host is read where it lies)
// 16-byte piece |g| of the paths: digest g / 2 is paths[q][l], the layer-l sibling of indices[q]'s ancestor
__host__ __device__ inline void merkle_open_item(mk_q* paths, const mk_q* tree, unsigned lg_n, const uint64_t* indices, size_t g)
{
    const size_t d = g >> 1, q = d / lg_n;
    const unsigned l = (unsigned)(d - q * lg_n);
    const size_t at = merkle_layer_offset(lg_n, l) + ((indices[q] >> l) ^ 1);
    paths[g] = tree[2 * at + (g & 1)];
}

#ifndef SPPARK_HOST_EMULATION
__global__ __launch_bounds__(MERKLE_NT)
void k_merkle_open(mk_q* paths, const mk_q* tree, unsigned lg_n, const uint64_t* indices, size_t pieces)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (size_t g = (size_t)blockIdx.x * MERKLE_NT + threadIdx.x; g < pieces; g += (size_t)gridDim.x * MERKLE_NT)
        merkle_open_item(paths, tree, lg_n, indices, g);
#endif
}
#endif

// word |g| of the rows: rows[q][j] = e(j, indices[q]), elements of |ew| words
__host__ __device__ inline void merkle_gather_item(u32* rows, const u32* in, size_t width, size_t col_stride, size_t leaf_stride, unsigned ew,
                                     const uint64_t* indices, size_t g)
{
    const size_t e = g / ew, w = g - e * ew, q = e / width, j = e - q * width;
    rows[g] = in[(j * col_stride + (size_t)indices[q] * leaf_stride) * ew + w];
}

#ifndef SPPARK_HOST_EMULATION
__global__ __launch_bounds__(MERKLE_NT)
void k_merkle_gather(u32* rows, const u32* in, size_t width, size_t col_stride, size_t leaf_stride, unsigned ew, const uint64_t* indices,
                     size_t nwords)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (size_t g = (size_t)blockIdx.x * MERKLE_NT + threadIdx.x; g < nwords; g += (size_t)gridDim.x * MERKLE_NT)
        merkle_gather_item(rows, in, width, col_stride, leaf_stride, ew, indices, g);
#endif
}
#endif

} // namespace sppark_amd
