// FRI on evaluation vectors (include/sppark_amd_fri.h): the arity-2^a fold, the points of the domain, and the weighted sum of
// a matrix's columns.  The reference has no counterpart.  The geometry is fri_route.hpp's.
//
// The domain is x = shift * w^E(i), w of order n = 2^lg_n: E(i) = i (NATURAL) or bitrev_lg_n(i) (BITREV).
//
//   k_fri_fold     one result is the group of A = 2^a inputs that a single folds reduce to it.  BITREV: in[A k .. A k + A);
//                  NATURAL: in[k + s m], m = n / A.  Read into v[] with the member index bit-reversed in NATURAL, both orders
//                  are the SAME computation (fri_fold_group): level l pairs (v[2t], v[2t+1]),
//                      v[t] = (lo + hi) + T_l[t] (lo - hi),   T_0[t] = beta / X_k * zeta^-bitrev(t),  T_(l+1)[t] = T_l[2t]^2
//                  with X_k the point of the group's first member, zeta = w^m of order A, and the a halvings as ONE product by
//                  2^-a at the end.  (beta / x of a level is the square of the one before: beta^2 and x^2.)
//   twiddles       1 / X_k = 1/shift * w^-E(k) is never read from memory.  k = tile 2^out_lg + e with e = (u 256 + t) N + j
//                  the lane's in-tile index, and E splits accordingly (fri_lane_exp, fri_const_exp, fri_tile_of):
//                      lane part   beta/shift * w^-(lane_exp) * c[u N + j], formed ONCE per lane and launch and held in
//                                  registers for every tile the lane visits.  lane_exp is a sum over the hexadecimal digits
//                                  of the lane and of the work-group, so w^-(lane_exp) is five products of entries of the
//                                  16-entry tables tt / tb, which the host passes by value (a launch of the 256-bit fields
//                                  carries 2.9 KB of arguments); then one product by a constant per result slot;
//                      tile part   one product by the host constant |step| per grid-stride step: NATURAL tiles b, b + G, ..
//                                  add G 2^out_lg to the exponent; BITREV visits tile b + G bitrev(s) in step s, which adds 1.
//                  No field_pow sits in the per-element path.
//   k_fri_domain   out[i] = x_i - z: the same split, going forward; one product and one subtraction per point.
//   k_fri_reduce   out[i] = (accumulate ? out[i] : 0) + sum_j weights[j] e(j, i) - sub.  Weights staged in LDS in chunks; the sum
//                  of a chunk goes through fri_acc, which for a bb31 matrix under bb31x4 weights is four 64-bit sums of 32 x 32
//                  products that are reduced once per FRI_LAZY_TERMS terms (the derivation is at fri_acc).
//
// The *_lane functions are the kernels' whole per-lane work; tests/emu/emu_fri.cpp runs them on the host for every
// (work-group, lane) of the route's grid.
#pragma once
#include "../ff/small_fields_dev.hpp"
#include "../mle/mle_kernels.hpp"
#include "fri_route.hpp"

namespace sppark_amd {

// the field the domain lives in: the library's own, except for the BabyBear quartic extension
template<class F> struct fri_base {
    typedef F type;
    SPPARK_DEVFN static F mulb(const F& a, const F& b) { return a * b; }
    SPPARK_DEVFN static F embed(const F& b) { return b; }
};
template<> struct fri_base<bb31_4_dev> {
    typedef bb31_dev type;
    SPPARK_DEVFN static bb31_4_dev mulb(const bb31_4_dev& a, const bb31_dev& b)
    {   bb31_4_dev r; for (int i = 0; i < 4; i++) r.c[i] = a.c[i] * b; return r;   }
    SPPARK_DEVFN static bb31_4_dev embed(const bb31_dev& b)
    {   bb31_4_dev r; r.c[0] = b; r.c[1] = r.c[2] = r.c[3] = bb31_dev::from_raw(0); return r;   }
};

// what the host computes for one launch, passed by value (B: the base field, CN: result slots per lane and tile)
template<class B, unsigned CN> struct fri_consts {
    B base;             // fold: 1 / shift; domain: shift
    B step;             // the tile part's factor per grid-stride step: r^fri_step_exp, r = w^-1 (fold) or w (domain)
    B scale;            // fold: 2^-a
    B z[4];             // fold: z[t] = zeta^-bitrev_(a-1)(t), t < 2^(a-1)
    B c[CN];            // c[u N + j] = r^fri_const_exp(u, j)
    B tt[2][16];        // tt[d][i] = r^fri_lane_exp(work-group 0, lane i 16^d)
    B tb[3][16];        // tb[d][i] = r^fri_lane_exp(work-group i 16^d, lane 0); one beyond the grid
};
static constexpr unsigned FRI_MAX_GRID_LG = 12;                     // three hexadecimal digits of a work-group's index
static_assert(FRI_NT == 256, "two hexadecimal digits of a lane's index");

// r^fri_lane_exp(b, t): the exponent is additive over the digits of b and of t (disjoint bit fields, reversed or not)
template<class B, unsigned CN>
SPPARK_DEVFN B fri_lane_power(const fri_consts<B, CN>& k, unsigned b, unsigned t)
{   return ((k.tt[0][t & 15] * k.tt[1][(t >> 4) & 15]) * (k.tb[0][b & 15] * k.tb[1][(b >> 4) & 15])) * k.tb[2][(b >> 8) & 15];   }
struct fri_geom { unsigned lg_m, out_lg, tile_bits, grid_lg; };     // log2 results, the route's tile and grid

// (index arithmetic the host needs as well, for the constants: api/fri_api.hpp)
#define SPPARK_FRI_HD __host__ __device__ inline
SPPARK_FRI_HD u64 fri_bitrev(u64 x, unsigned bits)
{
    u64 r = 0;
    for (unsigned i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}
// log2 results of a tile that exist (a vector below one tile)
SPPARK_FRI_HD unsigned fri_in_tile_bits(const fri_geom& g) { return g.out_lg < g.lg_m ? g.out_lg : g.lg_m; }
// the exponent of lane |t| of work-group |b| at its result slot 0 in step 0; |n_acc| results per access
SPPARK_FRI_HD u64 fri_lane_exp(bool bitrev, const fri_geom& g, unsigned b, unsigned t, unsigned n_acc)
{
    if (!bitrev) return ((u64)b << g.out_lg) + (u64)t * n_acc;
    return (fri_bitrev((u64)t * n_acc, fri_in_tile_bits(g)) << g.tile_bits) + (fri_bitrev(b, g.grid_lg) << (g.tile_bits - g.grid_lg));
}
// what slot (u, j) adds to it (0 for a slot beyond the vector: never used)
SPPARK_FRI_HD u64 fri_const_exp(bool bitrev, const fri_geom& g, unsigned u, unsigned j, unsigned n_acc)
{
    const u64 e = (u64)u * FRI_NT * n_acc + j;
    if (e >> fri_in_tile_bits(g)) return 0;
    return bitrev ? fri_bitrev(e, fri_in_tile_bits(g)) << g.tile_bits : e;
}
// what one step adds
SPPARK_FRI_HD u64 fri_step_exp(bool bitrev, const fri_geom& g) { return bitrev ? 1 : (u64)1 << (g.grid_lg + g.out_lg); }
// the tile of work-group |b| in step |s| < 2^(tile_bits - grid_lg)
SPPARK_FRI_HD size_t fri_tile_of(bool bitrev, const fri_geom& g, unsigned b, size_t s)
{   return bitrev ? b + ((size_t)fri_bitrev(s, g.tile_bits - g.grid_lg) << g.grid_lg) : b + (s << g.grid_lg);   }

// ---- fold ---------------------------------------------------------------------------------------------------------------
// the group v[0 .. 2^LGA) (NATURAL: member index bit-reversed) to its one result; tw = beta / X_k
template<class F, unsigned LGA>
SPPARK_DEVFN F fri_fold_group(F* v, const F& tw, const typename fri_base<F>::type* z, const typename fri_base<F>::type& scale)
{
    constexpr unsigned H = 1u << (LGA - 1);
    F T[H];
    T[0] = tw;
    #pragma unroll
    for (unsigned t = 1; t < H; t++) T[t] = fri_base<F>::mulb(tw, z[t]);
    #pragma unroll
    for (unsigned l = 0; l < LGA; l++) {
        #pragma unroll
        for (unsigned t = 0; t < (H >> l); t++) {
            const F lo = v[2 * t], hi = v[2 * t + 1];
            v[t] = (lo + hi) + T[t] * (lo - hi);
        }
        #pragma unroll
        for (unsigned t = 0; t < (H >> l) / 2; t++) T[t] = T[2 * t] * T[2 * t];
    }
    return fri_base<F>::mulb(v[0], scale);
}

template<class F, unsigned LGA, bool VEC> struct fri_fold_shape {
    static constexpr unsigned N = VEC ? fri_pack(sizeof(F)) : 1, U = fri_accesses(sizeof(F), LGA, N), CN = U * N;
};

// the whole work of lane |t| of work-group |block|
template<class F, unsigned LGA, bool BITREV, bool VEC>
SPPARK_DEVFN void fri_fold_lane(F* out, const F* in, const F& beta,
                                const fri_consts<typename fri_base<F>::type, fri_fold_shape<F, LGA, VEC>::CN>& k, const fri_geom& g,
                                unsigned block, unsigned t)
{
    typedef typename fri_base<F>::type B;
    typedef fri_fold_shape<F, LGA, VEC> S;
    constexpr unsigned N = S::N, U = S::U, A = 1u << LGA;
    typedef mle_chunk<F, N> chunk;
    const chunk* ci = reinterpret_cast<const chunk*>(in);
    chunk* co = reinterpret_cast<chunk*>(out);

    const B lb = k.base * fri_lane_power(k, block, t);
    F L[S::CN];
    #pragma unroll
    for (unsigned c = 0; c < S::CN; c++) L[c] = fri_base<F>::mulb(beta, lb * k.c[c]);
    B tp = B::one();

    const size_t nchunk = ((size_t)1 << g.lg_m) / N, steps = (size_t)1 << (g.tile_bits - g.grid_lg);
    for (size_t s = 0; s < steps; s++) {
        const size_t first = fri_tile_of(BITREV, g, block, s) * ((size_t)FRI_NT * U) + t;
        chunk V[U][A];
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = first + u * FRI_NT;
            if (i >= nchunk) continue;
            #pragma unroll
            for (unsigned q = 0; q < A; q++) V[u][q] = BITREV ? ci[i * A + q] : ci[i + q * nchunk];
        }
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = first + u * FRI_NT;
            if (i >= nchunk) continue;
            chunk R;
            #pragma unroll
            for (unsigned j = 0; j < N; j++) {
                F v[A];
                #pragma unroll
                for (unsigned q = 0; q < A; q++) {
                    if (BITREV) v[q] = V[u][(j * A + q) / N].e[(j * A + q) % N];        // group j of the A N contiguous elements
                    else        v[(unsigned)fri_bitrev(q, LGA)] = V[u][q].e[j];             // member q lies q m further on
                }
                R.e[j] = fri_fold_group<F, LGA>(v, fri_base<F>::mulb(L[u * N + j], tp), k.z, k.scale);
            }
            co[i] = R;
        }
        tp = tp * k.step;
    }
}

template<class F, unsigned LGA, bool BITREV, bool VEC>
__global__ __launch_bounds__(FRI_NT)
void k_fri_fold(F* out, const F* in, F bval, const F* bptr,
                fri_consts<typename fri_base<F>::type, fri_fold_shape<F, LGA, VEC>::CN> k, fri_geom g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    F beta = bval;
    if (bptr != nullptr) beta = *bptr;
    fri_fold_lane<F, LGA, BITREV, VEC>(out, in, beta, k, g, blockIdx.x, threadIdx.x);
#endif
}

// ---- domain -------------------------------------------------------------------------------------------------------------
template<class F, bool VEC> struct fri_domain_shape {
    static constexpr unsigned N = VEC ? fri_pack(sizeof(F)) : 1, U = fri_accesses(sizeof(F), 0, N), CN = U * N;
};

template<class F, bool BITREV, bool VEC>
SPPARK_DEVFN void fri_domain_lane(F* out, const F& z, const fri_consts<typename fri_base<F>::type, fri_domain_shape<F, VEC>::CN>& k,
                                  const fri_geom& g, unsigned block, unsigned t)
{
    typedef typename fri_base<F>::type B;
    typedef fri_domain_shape<F, VEC> S;
    constexpr unsigned N = S::N, U = S::U;
    typedef mle_chunk<F, N> chunk;
    chunk* co = reinterpret_cast<chunk*>(out);

    const B lb = k.base * fri_lane_power(k, block, t);
    B L[S::CN];
    #pragma unroll
    for (unsigned c = 0; c < S::CN; c++) L[c] = lb * k.c[c];
    B tp = B::one();

    const size_t nchunk = ((size_t)1 << g.lg_m) / N, steps = (size_t)1 << (g.tile_bits - g.grid_lg);
    for (size_t s = 0; s < steps; s++) {
        const size_t first = fri_tile_of(BITREV, g, block, s) * ((size_t)FRI_NT * U) + t;
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = first + u * FRI_NT;
            if (i >= nchunk) continue;
            chunk R;
            #pragma unroll
            for (unsigned j = 0; j < N; j++) R.e[j] = fri_base<F>::embed(L[u * N + j] * tp) - z;
            co[i] = R;
        }
        tp = tp * k.step;
    }
}

template<class F, bool BITREV, bool VEC>
__global__ __launch_bounds__(FRI_NT)
void k_fri_domain(F* out, F zval, const F* zptr, fri_consts<typename fri_base<F>::type, fri_domain_shape<F, VEC>::CN> k, fri_geom g)
{
#if defined(__HIP_DEVICE_COMPILE__)
    F z = zval;
    if (zptr != nullptr) z = *zptr;
    fri_domain_lane<F, BITREV, VEC>(out, z, k, g, blockIdx.x, threadIdx.x);
#endif
}

// ---- reduce -------------------------------------------------------------------------------------------------------------
// terms between two settle() calls, whatever the accumulator
static constexpr unsigned FRI_LAZY_TERMS = 4;

// sum_j w_j e_j over matrix elements e of type E under weights of type F; settle() at least every FRI_LAZY_TERMS terms
template<class F, class E> struct fri_acc {
    F s;
    SPPARK_DEVFN void init() { s = mle_zero<F>(); }
    SPPARK_DEVFN void add(const E& e, const F& w) { s = s + w * e; }
    SPPARK_DEVFN void settle() {}
    SPPARK_DEVFN F get() { return s; }
};
// A BabyBear matrix under quartic-extension weights: component c of the sum is sum_j e_j w_j[c] over Montgomery residues, and
// the Montgomery reduction of the SUM of the products is the sum of the Montgomery products.  So t[c] collects the 64-bit
// products e_j * w_j[c] (one v_mad_u64_u32 each) and is reduced lazily:
//   - every residue is canonical, so a product is at most PMAX = (p - 1)^2 = 0x3840000000000000 < 2^62;
//   - settle() replaces t by lo32(t) + hi32(t) * (2^32 mod p), congruent to t; 2^32 mod p = 0x0ffffffe, so afterwards
//     t <= SMAX = (2^32 - 1) * 0x0fffffff < 2^60;
//   - SMAX + k * PMAX <= 2^64 - 1 holds for k <= (2^64 - 1 - SMAX) / PMAX = 4: FRI_LAZY_TERMS, computed below, not tuned;
//   - get() settles once more and then Montgomery-reduces: t + m p < 2^60 + 2^32 p < 2^64, and the quotient is below
//     2^28 + p < 2 p, so one conditional subtraction makes it canonical.
template<> struct fri_acc<bb31_4_dev, bb31_dev> {
    static constexpr u64 P = bb31_dev::MOD, C32 = ((u64)1 << 32) % P;
    static constexpr u64 PMAX = (P - 1) * (P - 1), SMAX = 0xffffffffULL * (C32 + 1);
    static_assert(C32 == bb31_dev::ONE, "2^32 mod p");
    static_assert((~(u64)0 - SMAX) / PMAX == FRI_LAZY_TERMS, "terms per settle(): (2^64 - 1 - SMAX) / PMAX");
    static_assert(SMAX < ((u64)1 << 60) && (P << 32) < ~(u64)0 - ((u64)1 << 60), "get(): t + m p stays below 2^64");
    u64 t[4];
    SPPARK_DEVFN void init() { t[0] = t[1] = t[2] = t[3] = 0; }
    SPPARK_DEVFN void add(const bb31_dev& e, const bb31_4_dev& w)
    {
        #pragma unroll
        for (int c = 0; c < 4; c++) t[c] += (u64)e.v * w.c[c].v;
    }
    SPPARK_DEVFN void settle()
    {
        #pragma unroll
        for (int c = 0; c < 4; c++) t[c] = (u64)(u32)t[c] + (t[c] >> 32) * C32;
    }
    SPPARK_DEVFN bb31_4_dev get()
    {
        settle();
        bb31_4_dev r;
        #pragma unroll
        for (int c = 0; c < 4; c++) {
            const u32 m = (u32)t[c] * bb31_dev::M;
            const u32 q = (u32)((t[c] + (u64)m * P) >> 32);             // < 2 p
            r.c[c] = bb31_dev::from_raw(bb31_dev::umin(q, q - bb31_dev::MOD));
        }
        return r;
    }
};

// out[i] of leaf i: the chunk's sum on top of what is there (the call's first chunk: of out's old value or zero, less sub)
template<class F>
SPPARK_DEVFN void fri_reduce_store(F* out, size_t i, const F& sum, const F& sub, bool first, bool accumulate)
{
    F r = sum;
    if (!first || accumulate) r = out[i] + r;
    if (first) r = r - sub;
    out[i] = r;
}

// The leaves of lane |t| of work-group |block| over the |cw| columns from |j0| on, whose weights are wts[0 .. cw).
// COLS: NL = pack (VEC) or 1 leaves per lane, one access per column.  ROWS: one leaf per lane, pieces of pack (VEC) or 1
// elements along it.
template<class F, class E, bool COLS, bool VEC>
SPPARK_DEVFN void fri_reduce_lane(F* out, const E* in, const F* wts, size_t n, size_t j0, unsigned cw, size_t cs, size_t ls,
                                  const F& sub, bool first, bool accumulate, unsigned block, unsigned nblocks, unsigned t)
{
    constexpr unsigned P = VEC ? fri_pack(sizeof(E)) : 1;
    static_assert(P <= FRI_LAZY_TERMS, "an access is settled as a whole");
    typedef mle_chunk<E, P> chunk;
    typedef fri_acc<F, E> acc_t;
    if (COLS) {
        const size_t nq = n / P;
        for (size_t q = (size_t)block * FRI_NT + t; q < nq; q += (size_t)nblocks * FRI_NT) {
            const size_t i = q * P;
            acc_t acc[P];
            #pragma unroll
            for (unsigned l = 0; l < P; l++) acc[l].init();
            const E* col = in + j0 * cs + i;
            unsigned j = 0;
            for (; j + FRI_LAZY_TERMS <= cw; j += FRI_LAZY_TERMS) {
                chunk X[FRI_LAZY_TERMS];
                #pragma unroll
                for (unsigned d = 0; d < FRI_LAZY_TERMS; d++) X[d] = *reinterpret_cast<const chunk*>(col + (j + d) * cs);
                #pragma unroll
                for (unsigned l = 0; l < P; l++) {
                    #pragma unroll
                    for (unsigned d = 0; d < FRI_LAZY_TERMS; d++) acc[l].add(X[d].e[l], wts[j + d]);
                    acc[l].settle();
                }
            }
            for (; j < cw; j++) {                                       // at most FRI_LAZY_TERMS - 1 columns
                const chunk X = *reinterpret_cast<const chunk*>(col + j * cs);
                #pragma unroll
                for (unsigned l = 0; l < P; l++) acc[l].add(X.e[l], wts[j]);
            }
            #pragma unroll
            for (unsigned l = 0; l < P; l++) fri_reduce_store(out, i + l, acc[l].get(), sub, first, accumulate);
        }
    } else {
        constexpr unsigned G = FRI_LAZY_TERMS;                          // pieces loaded before the first is used
        for (size_t i = (size_t)block * FRI_NT + t; i < n; i += (size_t)nblocks * FRI_NT) {
            acc_t acc;
            acc.init();
            const E* row = in + i * ls + j0;
            unsigned j = 0;
            for (; j + G * P <= cw; j += G * P) {
                chunk X[G];
                #pragma unroll
                for (unsigned d = 0; d < G; d++) X[d] = *reinterpret_cast<const chunk*>(row + j + d * P);
                #pragma unroll
                for (unsigned d = 0; d < G; d++) {
                    #pragma unroll
                    for (unsigned e = 0; e < P; e++) acc.add(X[d].e[e], wts[j + d * P + e]);
                    if (P > 1) acc.settle();
                }
                acc.settle();
            }
            for (; j + P <= cw; j += P) {
                const chunk X = *reinterpret_cast<const chunk*>(row + j);
                #pragma unroll
                for (unsigned e = 0; e < P; e++) acc.add(X.e[e], wts[j + e]);
                acc.settle();
            }
            for (; j < cw; j++) acc.add(row[j], wts[j]);                // fewer than P <= FRI_LAZY_TERMS elements
            fri_reduce_store(out, i, acc.get(), sub, first, accumulate);
        }
    }
}

template<class F, class E, bool COLS, bool VEC>
__global__ __launch_bounds__(FRI_NT)
void k_fri_reduce(F* out, const E* in, const F* weights, size_t n, size_t width, size_t cs, size_t ls, F subval, const F* subptr,
                  int accumulate)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ F wts[FRI_RED_CHUNK];
    F sub = subval;
    if (subptr != nullptr) sub = *subptr;
    for (size_t j0 = 0; j0 < width; j0 += FRI_RED_CHUNK) {
        const unsigned cw = (unsigned)(width - j0 < FRI_RED_CHUNK ? width - j0 : FRI_RED_CHUNK);
        __syncthreads();
        for (unsigned j = threadIdx.x; j < cw; j += FRI_NT) wts[j] = weights[j0 + j];
        __syncthreads();
        fri_reduce_lane<F, E, COLS, VEC>(out, in, wts, n, j0, cw, cs, ls, sub, j0 == 0, accumulate != 0, blockIdx.x, gridDim.x, threadIdx.x);
    }
#endif
}

} // namespace sppark_amd
