// Poseidon2 over the library's field F (bb31_dev: width 16, gl64_dev: width 8): the permutation, the overwrite sponge over
// the leaves of a matrix, the binary tree above them.  The definition is include/sppark_amd_poseidon2.h; the tree's layout
// that of include/sppark_amd_merkle.h.  The reference's snapshot has no hash of any kind: nothing here is ported.
//
// This is field-multiplication code: 4 (RF T + RP) products for the S-boxes and RP T for the diagonal per permutation, all of
// them the bb31_dev / gl64_dev products of ff/small_fields_dev.hpp; the linear layers are additions only (M4 by the
// seven-addition chain below, 2 x and 3 x as sums).  One state per lane, in registers: every index into x[] is a
// compile-time constant -- the loops over the state have constant trip counts and are unrolled, the lane-local subtree of
// the nodes kernel is one template instance per node (merkle/merkle_kernels.hpp says why).  Only the loops over the rounds
// are left standing: their trip counts are the caller's and uniform.  tests/test_poseidon2_abi.py reads the code objects'
// metadata: no kernel here has a private segment.
//
// The constants are the caller's: |c| holds rounds_f * T external constants round by round, rounds_p internal constants and
// the T entries of the diagonal, in wire format.  Every index into it is uniform across the wave and the pointer is
// const __restrict__ down from the kernel's parameter, so the compiler may fetch the constants with scalar loads.
//
// Geometry (poseidon2_route.hpp): P2_NT lanes; a work-group strides over its items in steps of the grid.
//
//   k_p2_permute            one state of T elements (64 bytes) per lane, out == in allowed: a lane reads its state whole
//                           before it writes it.
//   k_p2_leaves<F, COLUMNS> one leaf per lane.  Element j of leaf i lies at (j * col_stride + i * leaf_stride) elements: in
//                           the columns layout the 64 lanes of a wave read 64 contiguous elements per load, in the rows
//                           layout a lane walks its own row.  A chunk of RATE elements overwrites x[0 .. RATE), an element
//                           past |width| leaves its position as it is; one permutation per chunk.
//   k_p2_nodes<F, S>        a lane reads 2^S consecutive digests of one layer (S = 3: 256 contiguous bytes), takes them down
//                           to one and writes every layer between.
//   k_p2_top<F>             one work-group takes a layer of at most P2_TOP digests to the root, level by level through two
//                           LDS buffers, writes every layer into the tree as well and the root to |root| if given.
//
// All offsets are 64-bit.  The *_lane / *_level functions are the kernels' bodies; tests/emu/emu_poseidon2.cpp runs them on
// the host for every (work-group, lane) of the route's grids.
#pragma once
#include "../ff/small_fields_dev.hpp"
#include "poseidon2_route.hpp"

namespace sppark_amd {

template<class F> struct p2_shape {
    static_assert(sizeof(F) == 4 || sizeof(F) == 8, "BabyBear (width 16) or Goldilocks (width 8)");
    static constexpr unsigned T = sizeof(F) == 4 ? 16 : 8, RATE = T / 2, OUT = T / 2;
};
template<class F> struct alignas(16) p2_digest { F e[p2_shape<F>::OUT]; };            // 32 bytes, moved as two 16-byte accesses
template<class F> struct alignas(16) p2_state { F e[p2_shape<F>::T]; };               // 64 bytes

// ---- the permutation -------------------------------------------------------------------------------------------------------
// x^7 = x^3 * x^4: four products
template<class F> SPPARK_DEVFN F p2_sbox(F x)
{
    const F x2 = x * x, x3 = x2 * x, x4 = x2 * x2;
    return x3 * x4;
}

// (a, b, c, d) <- M4 (a, b, c, d), M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]]: with s = a + b + c + d the rows are
// s + b + (a + b), s + b + 2 c, s + d + (c + d), s + d + 2 a
template<class F> SPPARK_DEVFN void p2_m4(F& a, F& b, F& c, F& d)
{
    const F ab = a + b, cd = c + d, s = ab + cd, sb = s + b, sd = s + d;
    const F y0 = sb + ab, y1 = sb + (c + c), y2 = sd + cd, y3 = sd + (a + a);
    a = y0; b = y1; c = y2; d = y3;
}

// M_E: z_b = M4 x_b per block of four, s = the sum of the z_b, y_b = z_b + s
template<class F, unsigned T> SPPARK_DEVFN void p2_external(F (&x)[T])
{
    #pragma unroll
    for (unsigned b = 0; b < T; b += 4) p2_m4(x[b], x[b + 1], x[b + 2], x[b + 3]);
    F s[4];
    #pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        s[k] = x[k];
        #pragma unroll
        for (unsigned b = 4; b < T; b += 4) s[k] = s[k] + x[b + k];
    }
    #pragma unroll
    for (unsigned i = 0; i < T; i++) x[i] = x[i] + s[i & 3];
}

// M_I: s = the sum of the x_i, y_i = d_i x_i + s
template<class F, unsigned T> SPPARK_DEVFN void p2_internal(F (&x)[T], const F* __restrict__ d)
{
    F s = x[0];
    #pragma unroll
    for (unsigned i = 1; i < T; i++) s = s + x[i];
    #pragma unroll
    for (unsigned i = 0; i < T; i++) x[i] = d[i] * x[i] + s;
}

template<class F, unsigned T> SPPARK_DEVFN void p2_full_rounds(F (&x)[T], const F* __restrict__ ce, unsigned rounds)
{
    for (unsigned r = 0; r < rounds; r++) {
        #pragma unroll
        for (unsigned i = 0; i < T; i++) x[i] = p2_sbox(x[i] + ce[(size_t)r * T + i]);
        p2_external<F, T>(x);
    }
}

template<class F> SPPARK_DEVFN void p2_permute(F (&x)[p2_shape<F>::T], const F* __restrict__ c, unsigned rf, unsigned rp)
{
    constexpr unsigned T = p2_shape<F>::T;
    const F* __restrict__ ci = c + (size_t)rf * T;
    const F* __restrict__ d = ci + rp;
    p2_external<F, T>(x);
    p2_full_rounds<F, T>(x, c, rf / 2);
    for (unsigned r = 0; r < rp; r++) {
        x[0] = p2_sbox(x[0] + ci[r]);
        p2_internal<F, T>(x, d);
    }
    p2_full_rounds<F, T>(x, c + (size_t)(rf / 2) * T, rf / 2);
}

// node: state = left || right, one permutation, the first OUT elements
template<class F> SPPARK_DEVFN void p2_node(p2_digest<F>& out, const p2_digest<F>& l, const p2_digest<F>& r, const F* __restrict__ c,
                                            unsigned rf, unsigned rp)
{
    constexpr unsigned OUT = p2_shape<F>::OUT;
    F x[p2_shape<F>::T];
    #pragma unroll
    for (unsigned i = 0; i < OUT; i++) { x[i] = l.e[i]; x[OUT + i] = r.e[i]; }
    p2_permute<F>(x, c, rf, rp);
    #pragma unroll
    for (unsigned i = 0; i < OUT; i++) out.e[i] = x[i];
}

// ---- permute: states in, states out ------------------------------------------------------------------------------------------
template<class F>
SPPARK_DEVFN void p2_permute_lane(p2_state<F>* out, const p2_state<F>* in, size_t count, const F* __restrict__ c, unsigned rf, unsigned rp,
                                  unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned T = p2_shape<F>::T;
    for (size_t i = (size_t)block * P2_NT + t; i < count; i += (size_t)nblocks * P2_NT) {
        const p2_state<F> s = in[i];
        F x[T];
        #pragma unroll
        for (unsigned k = 0; k < T; k++) x[k] = s.e[k];
        p2_permute<F>(x, c, rf, rp);
        p2_state<F> o;
        #pragma unroll
        for (unsigned k = 0; k < T; k++) o.e[k] = x[k];
        out[i] = o;
    }
}

// ---- leaves: the overwrite sponge -------------------------------------------------------------------------------------------
// the whole work of lane |t| of work-group |block| of |nblocks|: layer 0 of |tree|
template<class F, bool COLUMNS>
SPPARK_DEVFN void p2_leaf_lane(p2_digest<F>* tree, const F* in, size_t n, size_t width, size_t col_stride, size_t leaf_stride,
                               const F* __restrict__ c, unsigned rf, unsigned rp, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned T = p2_shape<F>::T, RATE = p2_shape<F>::RATE, OUT = p2_shape<F>::OUT;
    const size_t chunks = (width + RATE - 1) / RATE;
    for (size_t i = (size_t)block * P2_NT + t; i < n; i += (size_t)nblocks * P2_NT) {
        const F* p = in + (COLUMNS ? i : i * leaf_stride);
        F x[T];
        #pragma unroll
        for (unsigned k = 0; k < T; k++) x[k] = F::from_raw(0);
        for (size_t b = 0; b < chunks; b++) {
            #pragma unroll
            for (unsigned e = 0; e < RATE; e++) {
                const size_t j = b * RATE + e;
                if (j < width) x[e] = p[COLUMNS ? j * col_stride : j];
            }
            p2_permute<F>(x, c, rf, rp);
        }
        p2_digest<F> dg;
        #pragma unroll
        for (unsigned k = 0; k < OUT; k++) dg.e[k] = x[k];
        tree[i] = dg;
    }
}

// ---- nodes: lane-local subtrees ------------------------------------------------------------------------------------------------
// node K of level LV of a lane's subtree, then the nodes after it and the levels above (one instance per node: no index into
// d[] is computed at run time)
template<class F, unsigned S, unsigned LV, unsigned K>
SPPARK_DEVFN void p2_nodes_from(p2_digest<F> (&d)[1u << S], p2_digest<F>* tree, unsigned lg_n, unsigned first, size_t g,
                                const F* __restrict__ c, unsigned rf, unsigned rp)
{
    constexpr unsigned CNT = (1u << S) >> LV;
    p2_digest<F> r;
    p2_node<F>(r, d[2 * K], d[2 * K + 1], c, rf, rp);
    d[K] = r;
    tree[merkle_layer_offset(lg_n, first + LV) + g * CNT + K] = r;
    if constexpr (K + 1 < CNT) p2_nodes_from<F, S, LV, K + 1>(d, tree, lg_n, first, g, c, rf, rp);
    else if constexpr (LV < S) p2_nodes_from<F, S, LV + 1, 0>(d, tree, lg_n, first, g, c, rf, rp);
}

// lane |t| of work-group |block|: subtrees g of the |lanes| of layer |first|, 2^S digests in, layers first + 1 .. first + S out
template<class F, unsigned S>
SPPARK_DEVFN void p2_nodes_lane(p2_digest<F>* tree, unsigned lg_n, unsigned first, size_t lanes, const F* __restrict__ c, unsigned rf,
                                unsigned rp, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned C = 1u << S;
    for (size_t g = (size_t)block * P2_NT + t; g < lanes; g += (size_t)nblocks * P2_NT) {
        p2_digest<F> d[C];
        const p2_digest<F>* src = tree + merkle_layer_offset(lg_n, first) + g * C;
        #pragma unroll
        for (unsigned k = 0; k < C; k++) d[k] = src[k];
        p2_nodes_from<F, S, 1, 0>(d, tree, lg_n, first, g, c, rf, rp);
    }
}

// ---- top: one work-group to the root ---------------------------------------------------------------------------------------
// one level for lane |t|: |parents| digests from the 2 * parents at |src|, kept at |keep| (LDS) and written to |out| (the tree)
template<class F>
SPPARK_DEVFN void p2_top_level(p2_digest<F>* out, p2_digest<F>* keep, const p2_digest<F>* src, size_t parents, const F* __restrict__ c,
                               unsigned rf, unsigned rp, unsigned t)
{
    for (size_t i = t; i < parents; i += P2_NT) {
        p2_digest<F> r;
        p2_node<F>(r, src[2 * i], src[2 * i + 1], c, rf, rp);
        keep[i] = r;
        out[i] = r;
    }
}

#ifndef SPPARK_HOST_EMULATION
template<class F>
__global__ __launch_bounds__(P2_NT)
void k_p2_permute(p2_state<F>* out, const p2_state<F>* in, size_t count, const F* __restrict__ c, unsigned rf, unsigned rp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    p2_permute_lane<F>(out, in, count, c, rf, rp, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}

template<class F, bool COLUMNS>
__global__ __launch_bounds__(P2_NT)
void k_p2_leaves(p2_digest<F>* tree, const F* in, size_t n, size_t width, size_t col_stride, size_t leaf_stride, const F* __restrict__ c,
                 unsigned rf, unsigned rp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    p2_leaf_lane<F, COLUMNS>(tree, in, n, width, col_stride, leaf_stride, c, rf, rp, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}

template<class F, unsigned S>
__global__ __launch_bounds__(P2_NT)
void k_p2_nodes(p2_digest<F>* tree, unsigned lg_n, unsigned first, size_t lanes, const F* __restrict__ c, unsigned rf, unsigned rp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    p2_nodes_lane<F, S>(tree, lg_n, first, lanes, c, rf, rp, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}

template<class F>
__global__ __launch_bounds__(P2_NT)
void k_p2_top(p2_digest<F>* tree, p2_digest<F>* root, unsigned lg_n, unsigned first, const F* __restrict__ c, unsigned rf, unsigned rp)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ p2_digest<F> even[P2_TOP / 2], odd[P2_TOP / 4];               // the levels alternate between them
    const p2_digest<F>* src = tree + merkle_layer_offset(lg_n, first);
    for (unsigned l = first; l < lg_n; l++) {
        p2_digest<F>* keep = ((l - first) & 1) ? odd : even;
        p2_top_level<F>(tree + merkle_layer_offset(lg_n, l + 1), keep, src, (size_t)1 << (lg_n - l - 1), c, rf, rp, threadIdx.x);
        __syncthreads();
        src = keep;
    }
    if (root != nullptr && threadIdx.x == 0) *root = *src;                   // (lg_n == first: the one digest of the layer)
#endif
}
#endif

} // namespace sppark_amd
