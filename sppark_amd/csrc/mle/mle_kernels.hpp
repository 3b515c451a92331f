// Multilinear tables and sumcheck rounds (include/sppark_amd_mle.h): fold, evaluate, eq, round.  The reference has no
// counterpart: its callers' sumcheck provers keep their tables on the host.
//
// A table f has n = 2^lg_n canonical elements; index i = sum_j i_j 2^j, variable j is bit j.  The one operation under all
// four is the line through a pair, lo + r (hi - lo) (mle_line): one product.
//
// Geometry (mle_route.hpp): MLE_NT lanes, tiles of 2^T elements, 64 bytes per lane; a lane's elements are E / N accesses
// of N elements (N = 16 bytes' worth for the single-word fields; N = 1 in the element-wise instance, VEC == false, which a
// pointer that misses 16-byte alignment or a table below one access takes), access u of lane t being chunk u * MLE_NT + t
// of the tile.  Element e of a tile is therefore (u, t, j) with e = (u * MLE_NT + t) * N + j: the low lg N variables and
// the top lg U ones live in the lane's registers, the 8 between them in the lane index.  A lane issues every load of an
// iteration before the first use, and a work-group strides over tiles in steps of the grid.
//
//   k_mle_fold          out[i] = lo_i + r (hi_i - lo_i): streaming, no LDS.  LOW: a lane reads two consecutive accesses,
//                       which hold N whole pairs; HIGH: the same access of both halves.  HIGH may run in place: a lane
//                       writes only slots of the low half that it has read itself.
//   k_mle_bind          evaluate: one pass binds the tl variables of a tile.  Binding commutes (the extension is
//                       multilinear and the arithmetic exact), so the order inside a tile is free: the variables in the
//                       lane's registers first, six across the wave by lane exchange, two across the waves through LDS.
//                       One element per tile goes to the next pass.
//   k_mle_eq            out[i] = prod_j (i_j ? p_j : 1 - p_j).  The factor of the tl low variables does not depend on the
//                       tile: a lane forms it once for its E elements -- x (1 - p) = x - x p, one product per element --
//                       and every tile costs one product per element by the factor of the tile's index, which a wave
//                       forms itself: lane l takes variable tl + l, a product across the lanes follows.
//   k_sumcheck_round    every lane accumulates its d + 1 sums over its pairs; wave sum, work-group sum, one slab row per
//                       work-group.  k_sumcheck_sum, one work-group, adds the rows.  Field addition is exact and
//                       associative: the result does not depend on the grid.  The evaluation points t = 0 .. d are
//                       reached by adding hi - lo.
//
// The *_lane / *_pair / *_waves functions are the kernels' phases; tests/emu/emu_mle.cpp runs them on the host for every
// (work-group, lane) of the route's grids.  The arithmetic is the field classes' own operator+ - *.
#pragma once
#include "../poly/poly_kernels.hpp"
#include "mle_route.hpp"
#include <type_traits>

namespace sppark_amd {

enum { SUMCHECK_PRODUCT = 0, SUMCHECK_EQ_MUL_SUB = 1 };
static constexpr unsigned SUMCHECK_MAX_TABLES = 4, SUMCHECK_MAX_ROWS = 5;

template<class F> struct mle_geom {
    static constexpr unsigned PACK = mle_pack(sizeof(F));
    static constexpr unsigned T = mle_tile_lg(sizeof(F));
    static constexpr unsigned E = (1u << T) / MLE_NT;                       // elements per lane and tile: 16 / 8 / 4 / 2
};
static inline constexpr unsigned mle_lg(unsigned v) { return v <= 1 ? 0 : 1 + mle_lg(v >> 1); }

// N elements moved as one (16 bytes for the packed single-word fields)
template<class F, unsigned N> struct alignas(N * sizeof(F) >= 16 ? 16 : alignof(F)) mle_chunk { F e[N]; };

template<class F> struct mle_tables { const F* p[SUMCHECK_MAX_TABLES]; };

template<class F> SPPARK_DEVFN F mle_zero() { F r; __builtin_memset(&r, 0, sizeof(r)); return r; }           // every wire format: zero bits
template<class F> SPPARK_DEVFN F mle_line(const F& lo, const F& hi, const F& r) { return lo + r * (hi - lo); }

// ---- fold ---------------------------------------------------------------------------------------------------------------
// the whole work of lane |t| of work-group |block| of |nblocks|: |half| = n / 2 results
template<class F, bool HIGH, bool VEC>
SPPARK_DEVFN void mle_fold_lane(F* out, const F* in, const F& r, size_t half, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1;
    constexpr unsigned U = mle_geom<F>::E / N / 2;                          // result accesses per lane and tile
    typedef mle_chunk<F, N> chunk;
    const chunk* ci = reinterpret_cast<const chunk*>(in);
    chunk* co = reinterpret_cast<chunk*>(out);
    const size_t nchunk = half / N, step = (size_t)MLE_NT * U, stride = (size_t)nblocks * step;
    for (size_t base = (size_t)block * step; base < nchunk; base += stride) {
        chunk A[U], B[U];
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = base + u * MLE_NT + t;
            if (i >= nchunk) continue;
            A[u] = HIGH ? ci[i] : ci[2 * i];
            B[u] = HIGH ? ci[i + nchunk] : ci[2 * i + 1];
        }
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = base + u * MLE_NT + t;
            if (i >= nchunk) continue;
            chunk R;
            #pragma unroll
            for (unsigned j = 0; j < N; j++) {
                if (HIGH) R.e[j] = mle_line(A[u].e[j], B[u].e[j], r);
                else {                                                      // pair j of the 2N elements A ++ B
                    const F& lo = 2 * j < N ? A[u].e[(2 * j) % N] : B[u].e[(2 * j) % N];
                    const F& hi = 2 * j + 1 < N ? A[u].e[(2 * j + 1) % N] : B[u].e[(2 * j + 1) % N];
                    R.e[j] = mle_line(lo, hi, r);
                }
            }
            co[i] = R;
        }
    }
}

template<class F, bool HIGH, bool VEC, bool KPTR>
__global__ __launch_bounds__(MLE_NT)
void k_mle_fold(F* out, const F* in, F rval, const F* rptr, size_t half)
{
#if defined(__HIP_DEVICE_COMPILE__)
    F r = rval;
    if (KPTR) r = *rptr;
    mle_fold_lane<F, HIGH, VEC>(out, in, r, half, blockIdx.x, gridDim.x, threadIdx.x);
#endif
}

// ---- evaluate: one pass ---------------------------------------------------------------------------------------------------
// phase 1: lane |t| loads its elements of tile |tile| (2^tl elements at in + tile * 2^tl) and binds the variables that live
// in its registers; pt[b] is the value variable b OF THE TILE is bound to.  VEC: tl == T.
template<class F, bool VEC>
SPPARK_DEVFN F mle_bind_lane(const F* in, size_t tile, unsigned tl, const F* pt, unsigned t)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1, U = mle_geom<F>::E / N, LGN = mle_lg(N), LGU = mle_lg(U);
    typedef mle_chunk<F, N> chunk;
    const chunk* ci = reinterpret_cast<const chunk*>(in + (tile << tl));
    const size_t nchunk = ((size_t)1 << tl) / N;
    chunk X[U];
    #pragma unroll
    for (unsigned u = 0; u < U; u++) {
        const size_t i = (size_t)u * MLE_NT + t;
        if (i < nchunk) X[u] = ci[i];
        else { for (unsigned j = 0; j < N; j++) X[u].e[j] = mle_zero<F>(); }
    }
    #pragma unroll
    for (unsigned b = 0; b < LGN; b++) {                                    // the variables inside an access
        const F r = pt[b];
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            #pragma unroll
            for (unsigned i = 0; i < (N >> (b + 1)); i++) X[u].e[i] = mle_line(X[u].e[2 * i], X[u].e[2 * i + 1], r);
        }
    }
    #pragma unroll
    for (unsigned k = 0; k < LGU; k++) {                                    // the variables across the lane's accesses
        const unsigned bit = LGN + 8 + k;
        if (bit >= tl) break;
        const F r = pt[bit];
        #pragma unroll
        for (unsigned i = 0; i < (U >> (k + 1)); i++) X[i].e[0] = mle_line(X[2 * i].e[0], X[2 * i + 1].e[0], r);
    }
    return X[0].e[0];
}
// phase 2, one step of the lane exchange: |mine| and the value of the lane whose index differs in one bit; up: mine is hi
template<class F> SPPARK_DEVFN F mle_bind_pair(const F& mine, const F& other, bool up, const F& r)
{   return mle_line(up ? other : mine, up ? mine : other, r);   }
// the variable that lane bit s (0 .. 7) of a pass stands for
template<class F, bool VEC> SPPARK_DEVFN constexpr unsigned mle_lane_bit(unsigned s) { return mle_lg(VEC ? mle_geom<F>::PACK : 1) + s; }
// phase 3: the values of the four waves -> the tile's one element
template<class F, bool VEC>
SPPARK_DEVFN F mle_bind_waves(const F* w, unsigned tl, const F* pt)
{
    F a = w[0], b = w[2];
    const unsigned b6 = mle_lane_bit<F, VEC>(6), b7 = mle_lane_bit<F, VEC>(7);
    if (b6 < tl) { a = mle_line(w[0], w[1], pt[b6]); if (b7 < tl) b = mle_line(w[2], w[3], pt[b6]); }
    if (b7 < tl) a = mle_line(a, b, pt[b7]);
    return a;
}

#if defined(__HIP_DEVICE_COMPILE__)
template<class F> __device__ __forceinline__ F mle_shfl_xor(const F& v, unsigned mask)
{
    constexpr unsigned W = sizeof(F) / 4;
    unsigned w[W];
    __builtin_memcpy(w, &v, sizeof(F));
    #pragma unroll
    for (unsigned i = 0; i < W; i++) w[i] = (unsigned)__shfl_xor((int)w[i], (int)mask, 64);
    F r;
    __builtin_memcpy(&r, w, sizeof(F));
    return r;
}
#endif

template<class F, bool VEC>
__global__ __launch_bounds__(MLE_NT)
void k_mle_bind(F* out, const F* in, const F* pt, unsigned tl, size_t tiles)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ F lds[MLE_NT / 64];
    const unsigned t = threadIdx.x;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        F v = mle_bind_lane<F, VEC>(in, tile, tl, pt, t);
        #pragma unroll
        for (unsigned s = 0; s < 6; s++) {
            const unsigned bit = mle_lane_bit<F, VEC>(s);
            if (bit >= tl) break;
            v = mle_bind_pair(v, mle_shfl_xor(v, 1u << s), (t >> s) & 1, pt[bit]);
        }
        if ((t & 63) == 0) lds[t >> 6] = v;
        __syncthreads();
        if (t == 0) out[tile] = mle_bind_waves<F, VEC>(lds, tl, pt);
        __syncthreads();
    }
#endif
}

// ---- eq ---------------------------------------------------------------------------------------------------------------------
// the factor of the tile's tl low variables for every element of lane |t|
template<class F, bool VEC>
SPPARK_DEVFN void mle_eq_lane(mle_chunk<F, VEC ? mle_geom<F>::PACK : 1>* X, const F* point, unsigned tl, unsigned t)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1, U = mle_geom<F>::E / N, LGN = mle_lg(N), LGU = mle_lg(U);
    F a = F::one();
    #pragma unroll 1
    for (unsigned s = 0; s < 8; s++) {                                      // the lane's own index bits
        const unsigned bit = LGN + s;
        if (bit >= tl) break;
        const F ap = a * point[bit];
        a = ((t >> s) & 1) ? ap : a - ap;
    }
    X[0].e[0] = a;
    #pragma unroll
    for (unsigned b = 0; b < LGN; b++) {                                    // inside an access (VEC: tl == T > LGN)
        const F p = point[b];
        #pragma unroll
        for (unsigned i = 0; i < (1u << b); i++) {
            const F hi = X[0].e[i] * p;
            X[0].e[i + (1u << b)] = hi;
            X[0].e[i] = X[0].e[i] - hi;
        }
    }
    #pragma unroll
    for (unsigned k = 0; k < LGU; k++) {                                    // across the lane's accesses
        const unsigned bit = LGN + 8 + k;
        if (bit >= tl) break;
        const F p = point[bit];
        #pragma unroll
        for (unsigned i = 0; i < (1u << k); i++) {
            #pragma unroll
            for (unsigned j = 0; j < N; j++) {
                const F hi = X[i].e[j] * p;
                X[i + (1u << k)].e[j] = hi;
                X[i].e[j] = X[i].e[j] - hi;
            }
        }
    }
}
// exchange steps that cover |nhigh| lanes: the least s with 2^s >= nhigh
SPPARK_DEVFN unsigned mle_eq_steps(unsigned nhigh) { unsigned s = 0; while ((1u << s) < nhigh) s++; return s; }
// Every group of 2^steps lanes of a wave forms the tile's factor: lane |l| of a group takes variable tl + l (one beyond the
// last variable); p = point[tl + l], q = 1 - p
template<class F> SPPARK_DEVFN F mle_eq_factor(const F& p, const F& q, unsigned nhigh, size_t tile, unsigned l)
{   return l < nhigh ? (((tile >> l) & 1) ? p : q) : F::one();   }
// the lane's accesses of tile |tile|, each element times |pre| (nhigh == 0: as they are)
template<class F, bool VEC>
SPPARK_DEVFN void mle_eq_store(F* out, const mle_chunk<F, VEC ? mle_geom<F>::PACK : 1>* X, const F& pre, unsigned nhigh, size_t tile,
                               unsigned tl, unsigned t)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1, U = mle_geom<F>::E / N;
    typedef mle_chunk<F, N> chunk;
    chunk* co = reinterpret_cast<chunk*>(out + (tile << tl));
    const size_t nchunk = ((size_t)1 << tl) / N;
    #pragma unroll
    for (unsigned u = 0; u < U; u++) {
        const size_t i = (size_t)u * MLE_NT + t;
        if (i >= nchunk) continue;
        chunk R = X[u];
        if (nhigh) {
            #pragma unroll
            for (unsigned j = 0; j < N; j++) R.e[j] = X[u].e[j] * pre;
        }
        co[i] = R;
    }
}

template<class F, bool VEC>
__global__ __launch_bounds__(MLE_NT)
void k_mle_eq(F* out, const F* point, unsigned lg_n, unsigned tl, size_t tiles)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1, U = mle_geom<F>::E / N;
    const unsigned t = threadIdx.x, nhigh = lg_n - tl, steps = mle_eq_steps(nhigh), l = t & ((1u << steps) - 1);
    mle_chunk<F, N> X[U];
    mle_eq_lane<F, VEC>(X, point, tl, t);
    F p = F::one(), q = F::one();
    if (l < nhigh) { p = point[tl + l]; q = F::one() - p; }
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        F pre = mle_eq_factor(p, q, nhigh, tile, l);
        #pragma unroll 1
        for (unsigned s = 0; s < steps; s++) pre = pre * mle_shfl_xor(pre, 1u << s);
        mle_eq_store<F, VEC>(out, X, pre, nhigh, tile, tl, t);
    }
#endif
}

// ---- round ------------------------------------------------------------------------------------------------------------------
template<int NTAB, int FORM> struct sumcheck_shape { static constexpr unsigned ROWS = FORM == SUMCHECK_EQ_MUL_SUB ? 4 : NTAB + 1; };

// one pair of every table into the ROWS sums: s(t) += form(f_k(t)), f_k(t) = lo_k + t (hi_k - lo_k), t by repeated addition.
// Row by row through a template, not a loop: every index into acc, f, d is a constant whatever the unroller decides.
template<class F, int NTAB, int FORM, unsigned R>
SPPARK_DEVFN void sumcheck_row(F* acc, F* f, const F* d, const F* hi)
{
    if (R == 1) {
        #pragma unroll
        for (int k = 0; k < NTAB; k++) f[k] = hi[k];
    } else if (R > 1) {
        #pragma unroll
        for (int k = 0; k < NTAB; k++) f[k] = f[k] + d[k];
    }
    F term;
    if (FORM == SUMCHECK_EQ_MUL_SUB) term = f[0] * (f[1] * f[NTAB > 2 ? 2 : 0] - f[NTAB > 3 ? 3 : 0]);
    else {
        term = f[0];
        #pragma unroll
        for (int k = 1; k < NTAB; k++) term = term * f[k];
    }
    acc[R] = acc[R] + term;
    if constexpr (R + 1 < sumcheck_shape<NTAB, FORM>::ROWS) sumcheck_row<F, NTAB, FORM, R + 1>(acc, f, d, hi);
}
template<class F, int NTAB, int FORM>
SPPARK_DEVFN void sumcheck_pair(F* acc, const F* lo, const F* hi)
{
    F f[NTAB], d[NTAB];
    #pragma unroll
    for (int k = 0; k < NTAB; k++) { f[k] = lo[k]; d[k] = hi[k] - lo[k]; }
    sumcheck_row<F, NTAB, FORM, 0>(acc, f, d, hi);
}

// access u of an iteration into the sums, then the next one (a template, as sumcheck_row: the 15 extension-field products of
// a pair of four tables are beyond what "#pragma unroll" unrolls, and a rolled loop would index A and B in memory)
template<class F, int NTAB, int FORM, bool HIGH, unsigned N, unsigned U, unsigned u>
SPPARK_DEVFN void sumcheck_access(F* acc, const mle_chunk<F, N> (*A)[U], const mle_chunk<F, N> (*B)[U], size_t first, size_t nchunk)
{
    if (first + u * MLE_NT < nchunk) {
        #pragma unroll
        for (unsigned j = 0; j < N; j++) {
            F lo[NTAB], hi[NTAB];
            #pragma unroll
            for (int k = 0; k < NTAB; k++) {
                if (HIGH) { lo[k] = A[k][u].e[j]; hi[k] = B[k][u].e[j]; }
                else {
                    lo[k] = 2 * j < N ? A[k][u].e[(2 * j) % N] : B[k][u].e[(2 * j) % N];
                    hi[k] = 2 * j + 1 < N ? A[k][u].e[(2 * j + 1) % N] : B[k][u].e[(2 * j + 1) % N];
                }
            }
            sumcheck_pair<F, NTAB, FORM>(acc, lo, hi);
        }
    }
    if constexpr (u + 1 < U) sumcheck_access<F, NTAB, FORM, HIGH, N, U, u + 1>(acc, A, B, first, nchunk);
}

// the ROWS sums of lane |t| of work-group |block| over its pairs; |half| = n / 2 pairs per table
template<class F, int NTAB, int FORM, bool HIGH, bool VEC>
SPPARK_DEVFN void sumcheck_round_lane(F* acc, const mle_tables<F>& tabs, size_t half, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1;
    constexpr unsigned U = mle_geom<F>::E / N / 2;                          // accesses of N pairs per lane and tile
    constexpr unsigned ROWS = sumcheck_shape<NTAB, FORM>::ROWS;
    typedef mle_chunk<F, N> chunk;
    #pragma unroll
    for (unsigned r = 0; r < ROWS; r++) acc[r] = mle_zero<F>();
    const size_t nchunk = half / N, step = (size_t)MLE_NT * U, stride = (size_t)nblocks * step;
    for (size_t base = (size_t)block * step; base < nchunk; base += stride) {
        chunk A[NTAB][U], B[NTAB][U];
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = base + u * MLE_NT + t;
            if (i >= nchunk) continue;
            #pragma unroll
            for (int k = 0; k < NTAB; k++) {
                const chunk* ci = reinterpret_cast<const chunk*>(tabs.p[k]);
                A[k][u] = HIGH ? ci[i] : ci[2 * i];
                B[k][u] = HIGH ? ci[i + nchunk] : ci[2 * i + 1];
            }
        }
        sumcheck_access<F, NTAB, FORM, HIGH, N, U, 0>(acc, A, B, base + t, nchunk);
    }
}
// the ROWS (at most |rows|) sums of lane |t| of the one work-group over the slab's |nrows| rows
template<class F>
SPPARK_DEVFN void sumcheck_sum_lane(F* acc, const F* slab, size_t nrows, unsigned rows, unsigned t)
{
    #pragma unroll
    for (unsigned c = 0; c < SUMCHECK_MAX_ROWS; c++) acc[c] = mle_zero<F>();
    for (size_t i = t; i < nrows; i += MLE_NT) {
        #pragma unroll
        for (unsigned c = 0; c < SUMCHECK_MAX_ROWS; c++) if (c < rows) acc[c] = acc[c] + slab[i * rows + c];
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
// dst[c] = the sum of acc[c] over the work-group's lanes, c < ROWS
template<class F, unsigned ROWS>
__device__ __forceinline__ void sumcheck_block_sum(F* dst, F* acc, F* lds, unsigned t)
{
    #pragma unroll
    for (unsigned c = 0; c < ROWS; c++) {
        #pragma unroll 1
        for (unsigned s = 0; s < 6; s++) acc[c] = acc[c] + mle_shfl_xor(acc[c], 1u << s);
    }
    if ((t & 63) == 0) {
        #pragma unroll
        for (unsigned c = 0; c < ROWS; c++) lds[(t >> 6) * ROWS + c] = acc[c];
    }
    __syncthreads();
    if (t < ROWS) dst[t] = (lds[t] + lds[ROWS + t]) + (lds[2 * ROWS + t] + lds[3 * ROWS + t]);
}
#endif

template<class F, int NTAB, int FORM, bool HIGH, bool VEC>
__global__ __launch_bounds__(MLE_NT)
void k_sumcheck_round(F* slab, mle_tables<F> tabs, size_t half)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned ROWS = sumcheck_shape<NTAB, FORM>::ROWS;
    __shared__ F lds[(MLE_NT / 64) * ROWS];
    F acc[ROWS];
    sumcheck_round_lane<F, NTAB, FORM, HIGH, VEC>(acc, tabs, half, blockIdx.x, gridDim.x, threadIdx.x);
    sumcheck_block_sum<F, ROWS>(slab + (size_t)blockIdx.x * ROWS, acc, lds, threadIdx.x);
#endif
}

template<class F>
__global__ __launch_bounds__(MLE_NT)
void k_sumcheck_sum(F* out, const F* slab, size_t nrows, unsigned rows)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ F lds[(MLE_NT / 64) * SUMCHECK_MAX_ROWS];
    __shared__ F res[SUMCHECK_MAX_ROWS];
    F acc[SUMCHECK_MAX_ROWS];
    sumcheck_sum_lane(acc, slab, nrows, rows, threadIdx.x);
    sumcheck_block_sum<F, SUMCHECK_MAX_ROWS>(res, acc, lds, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < rows) out[threadIdx.x] = res[threadIdx.x];
#endif
}

} // namespace sppark_amd
