// Field-vector inverse and quotient: the role of the reference's ff/batch_inversion.hpp (Montgomery's
// trick: many inverses for ONE field inversion, zero mapped to zero), on a whole device array.
//
// The three launches and the tiling of the scans (poly_kernels.hpp: POLY_NT lanes of poly_geom<F>::E
// consecutive elements per tile, kernel boundaries as the only grid-wide synchronisation):
//
//   reduce    agg[tile] = product of the tile's elements                          (1 read of the array)
//   spine     one work-group: agg[tile] -> 1 / agg[tile] in place; the call's ONE field inversion
//   apply     every tile reloads its elements and turns 1 / (tile product) into the inverse of
//             each of them                                                        (1 read + 1 write)
//
// Zero: an element that is zero enters every product as one and its output is zero.  Every partial
// product is then non-zero (also that of an all-zero tile or array), the inversion never sees zero,
// and nothing else has to know about zeros.
//
// The step across the lanes of a tile (and of the spine) is a product tree in LDS: the up-sweep keeps
// every level (2*NT - 1 nodes in the 2*NT values the scans already ask for), the root is replaced by
// its inverse, and the down-sweep turns 1/parent into 1/left = (1/parent)*right and 1/right =
// (1/parent)*left.  3*(NT - 1) products per tree; two Hillis-Steele scans (prefix and suffix
// products) would take 16*NT.
//
// Products per element, E elements per lane: reduce (E-1)/E + 1/E (tree), apply 3*(E-1)/E + 3/E,
// i.e. 4 for both tile shapes (E = 8 and E = 4), plus one for the quotient; the spine adds 3 per TILE.
#pragma once
#include "poly_kernels.hpp"

namespace sppark_amd {

#if defined(__HIP_DEVICE_COMPILE__)
static constexpr unsigned INV_ROOT = 2 * POLY_NT - 2;           // level l of the tree starts at 2*NT - (2*NT >> l)

// leaves tree[0..NT) = one value per lane; every level above = products of pairs; tree[INV_ROOT] = all of them
template<class F>
__device__ __forceinline__ void inv_tree_up(const F& v, F* tree, unsigned t)
{
    tree[t] = v;
    __syncthreads();
    unsigned off = 0;
    #pragma unroll 1
    for (unsigned n = POLY_NT / 2; n; n >>= 1) {                // n nodes on the level being built, 2n below it at |off|
        if (t < n) tree[off + 2 * n + t] = tree[off + 2 * t] * tree[off + 2 * t + 1];
        __syncthreads();
        off += 2 * n;
    }
}
// tree[INV_ROOT] holds the INVERSE of the root: every node becomes its own inverse, level by level;
// returns the inverse of lane t's leaf
template<class F>
__device__ __forceinline__ F inv_tree_down(F* tree, unsigned t)
{
    unsigned off = INV_ROOT;
    #pragma unroll 1
    for (unsigned n = 1; n < POLY_NT; n <<= 1) {                // n inverted parents at |off|, their 2n children below
        const unsigned child = off - 2 * n;
        F mine = F::one();
        if (t < 2 * n) mine = tree[off + (t >> 1)] * tree[child + (t ^ 1)];     // 1/parent * sibling
        __syncthreads();                                        // (the sibling reads this node's old value)
        if (t < 2 * n) tree[child + t] = mine;
        __syncthreads();
        off = child;
    }
    return tree[t];
}

// the lane's E elements with zeros replaced by one; bit k of the result: element k was zero (or is past the end)
template<class F, unsigned E>
__device__ __forceinline__ unsigned inv_load(F (&x)[E], const F* inp, size_t base, size_t len)
{
    unsigned skip = 0;
    #pragma unroll
    for (unsigned k = 0; k < E; k++) {
        bool z = true;
        if (base + k < len) { x[k] = inp[base + k]; z = x[k].is_zero(); }
        if (z) { x[k] = F::one(); skip |= 1u << k; }
    }
    return skip;
}
#endif

// reduce: agg[tile] = product of the tile's elements (zeros as one)
template<class F>
__global__ __launch_bounds__(POLY_NT)
void k_inv_reduce(F* __restrict__ agg, const F* __restrict__ inp, size_t len)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned E = poly_geom<F>::E;
    extern __shared__ __attribute__((aligned(16))) unsigned char inv_lds[];
    F* tree = reinterpret_cast<F*>(inv_lds);
    const unsigned t = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * POLY_NT + t) * E;
    F x[E];
    (void)inv_load<F, E>(x, inp, base, len);
    F v = x[0];
    #pragma unroll
    for (unsigned k = 1; k < E; k++) v = v * x[k];
    inv_tree_up(v, tree, t);
    if (t == 0) agg[blockIdx.x] = tree[INV_ROOT];
#endif
}

// spine: agg[0..ntiles) -> their inverses, in place, one work-group of NT lanes over consecutive tiles per lane
// (as k_poly_spine); pre[0..ntiles) is scratch for a lane's running products.  The only inverse() of a call.
template<class F>
__global__ __launch_bounds__(POLY_NT)
void k_inv_spine(F* __restrict__ agg, F* __restrict__ pre, size_t ntiles)
{
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char inv_lds[];
    F* tree = reinterpret_cast<F*>(inv_lds);
    const unsigned t = threadIdx.x;
    const size_t per = (ntiles + POLY_NT - 1) / POLY_NT;
    const size_t lo = (size_t)t * per, hi = lo + per < ntiles ? lo + per : ntiles;
    F run = F::one();
    for (size_t i = lo; i < hi; i++) { pre[i] = run; run = run * agg[i]; }     // pre[i] = product of the lane's tiles before i
    inv_tree_up(run, tree, t);
    if (t == 0) tree[INV_ROOT] = tree[INV_ROOT].inverse();      // non-zero: a product of non-zero values
    __syncthreads();
    F inv = inv_tree_down(tree, t);                             // 1 / (product of the lane's tiles)
    for (size_t i = hi; i-- > lo;) { const F a = agg[i]; agg[i] = inv * pre[i]; inv = inv * a; }
#endif
}

// apply: out[i] = 1 / den[i] (DIV: num[i] / den[i]), 0 where den[i] == 0; tile_inv[tile] = 1 / (the tile's product).
// out may be den or num: a lane writes only the slots it has read.
template<class F, bool DIV>
__global__ __launch_bounds__(POLY_NT)
void k_inv_apply(F* out, const F* num, const F* den, const F* __restrict__ tile_inv, size_t len)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned E = poly_geom<F>::E;
    extern __shared__ __attribute__((aligned(16))) unsigned char inv_lds[];
    F* tree = reinterpret_cast<F*>(inv_lds);
    const unsigned t = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * POLY_NT + t) * E;
    F x[E], nm[DIV ? E : 1];
    const unsigned skip = inv_load<F, E>(x, den, base, len);
    if (DIV) {
        #pragma unroll
        for (unsigned k = 0; k < E; k++) if (base + k < len) nm[k] = num[base + k];
    }
    F p[E];                                                     // p[k] = x[0] * ... * x[k]
    p[0] = x[0];
    #pragma unroll
    for (unsigned k = 1; k < E; k++) p[k] = p[k - 1] * x[k];
    inv_tree_up(p[E - 1], tree, t);
    if (t == 0) tree[INV_ROOT] = tile_inv[blockIdx.x];
    __syncthreads();
    F inv = inv_tree_down(tree, t);                             // 1 / p[E-1]
    #pragma unroll
    for (unsigned k = E; k--;) {
        F y = inv;                                              // 1 / p[k]
        if (k) { y = inv * p[k - 1]; inv = inv * x[k]; }        // 1 / x[k];  1 / p[k-1]
        if (base + k < len) {
            if (DIV) y = y * nm[k];
            out[base + k] = ((skip >> k) & 1) ? poly_zero<F>() : y;
        }
    }
#endif
}

} // namespace sppark_amd
