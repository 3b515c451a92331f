// Field-vector arithmetic: out = a + b, a - b, a * b, a * k, (a * b - c) [* k], element by element over a whole
// device array -- what sits between two transforms of a prover (include/sppark_amd_arith.h).  The reference has no
// counterpart: its callers write such loops themselves, over the same wire formats.
//
// Streaming kernels: no LDS, no scratch, one read of every operand and one write.
//
//   access    16 bytes per lane and access: two Goldilocks words, four 31-bit words, one bb31_4 element, half a
//             256-bit element (whole elements per lane, two accesses each).  When one of the pointers is not 16-byte
//             aligned -- a view that starts at an odd element offset -- the single-word fields take the element-wise
//             instance (VEC == false) instead; never a misaligned 16-byte access.
//   in flight a lane loads ALL operands of its vec_geom<F>::U accesses of an iteration before the first use:
//             2 or 3 operands x U independent 16-byte loads (x 2 for the 256-bit fields).
//   grid      VEC_WG_PER_CU work-groups per CU at most, each striding over the array in steps of
//             gridDim.x * vec_geom<F>::T elements; T = elements one work-group handles per iteration.
//   aliasing  out may be any of the inputs, and inputs may be each other: a lane writes only slots it has read,
//             after it has read every operand of the iteration, and no pointer is __restrict__.
//
// k: by value (the caller's pointer was a host pointer) or read through the pointer (KPTR: a device pointer), the
// same for every lane.  The arithmetic is the field classes' own operator+ - *: canonical in, canonical out.
#pragma once
#include "poly_kernels.hpp"
#include "../util/runtime.hpp"
#include <algorithm>
#include <type_traits>

namespace sppark_amd {

enum vec_op : int { VEC_ADD = 0, VEC_SUB = 1, VEC_MUL = 2, VEC_SCALE = 3, VEC_MUL_SUB = 4, VEC_MUL_SUB_K = 5 };

static constexpr unsigned VEC_NT = 256;             // lanes per work-group
static constexpr unsigned VEC_WG_PER_CU = 8;        // the grid's cap: work-groups per CU

template<class F> struct vec_geom {
    static constexpr unsigned PACK = sizeof(F) < 16 ? 16 / sizeof(F) : 1;       // elements per 16-byte access
    static constexpr unsigned U = sizeof(F) <= 16 ? 4 : 2;                      // independent accesses (256-bit: elements) per lane and iteration
    static constexpr unsigned T = VEC_NT * U * PACK;                            // elements per work-group and iteration: 2048 / 4096 / 1024 / 512
};

// N elements moved as one: 16 bytes, 16-byte aligned, for the packed single-word fields; one element otherwise
template<class F, unsigned N> struct alignas(N * sizeof(F) >= 16 ? 16 : alignof(F)) vec_chunk { F e[N]; };

template<int OP> struct vec_uses {
    static constexpr bool B = OP != VEC_SCALE, C = OP == VEC_MUL_SUB || OP == VEC_MUL_SUB_K, K = OP == VEC_SCALE || OP == VEC_MUL_SUB_K;
};

template<int OP, class F>
SPPARK_DEVFN F vec_apply(const F& a, const F& b, const F& c, const F& k)
{
    if (OP == VEC_ADD) return a + b;
    if (OP == VEC_SUB) return a - b;
    if (OP == VEC_MUL) return a * b;
    if (OP == VEC_SCALE) return a * k;
    if (OP == VEC_MUL_SUB) return a * b - c;
    return (a * b - c) * k;
}

// VEC: every pointer is 16-byte aligned (always, for elements of 16 bytes and more)
template<class F, int OP, bool VEC, bool KPTR>
__global__ __launch_bounds__(VEC_NT)
void k_vec(F* out, const F* a, const F* b, const F* c, F kval, const F* kptr, size_t len)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned N = VEC ? vec_geom<F>::PACK : 1;                     // elements per access
    constexpr unsigned U = vec_geom<F>::T / (VEC_NT * N);                   // accesses per lane and iteration
    typedef vec_chunk<F, N> chunk;
    typedef vec_uses<OP> uses;
    const unsigned t = threadIdx.x;
    F k = kval;
    if (uses::K && KPTR) k = *kptr;
    const chunk* ca = reinterpret_cast<const chunk*>(a);
    const chunk* cb = reinterpret_cast<const chunk*>(b);
    const chunk* cc = reinterpret_cast<const chunk*>(c);
    chunk* co = reinterpret_cast<chunk*>(out);
    const size_t nchunk = len / N, step = (size_t)VEC_NT * U, stride = (size_t)gridDim.x * step;
    for (size_t base = (size_t)blockIdx.x * step; base < nchunk; base += stride) {
        chunk A[U], B[uses::B ? U : 1], C[uses::C ? U : 1];
        const size_t i0 = base + t;
        if (base + step <= nchunk) {                                        // a whole tile: nothing to guard
            #pragma unroll
            for (unsigned u = 0; u < U; u++) {
                A[u] = ca[i0 + u * VEC_NT];
                if (uses::B) B[u] = cb[i0 + u * VEC_NT];
                if (uses::C) C[u] = cc[i0 + u * VEC_NT];
            }
            #pragma unroll
            for (unsigned u = 0; u < U; u++) {
                chunk R;
                #pragma unroll
                for (unsigned j = 0; j < N; j++)
                    R.e[j] = vec_apply<OP>(A[u].e[j], B[uses::B ? u : 0].e[j], C[uses::C ? u : 0].e[j], k);
                co[i0 + u * VEC_NT] = R;
            }
        } else {
            #pragma unroll
            for (unsigned u = 0; u < U; u++) {
                if (i0 + u * VEC_NT >= nchunk) continue;
                A[u] = ca[i0 + u * VEC_NT];
                if (uses::B) B[u] = cb[i0 + u * VEC_NT];
                if (uses::C) C[u] = cc[i0 + u * VEC_NT];
            }
            #pragma unroll
            for (unsigned u = 0; u < U; u++) {
                if (i0 + u * VEC_NT >= nchunk) continue;
                chunk R;
                #pragma unroll
                for (unsigned j = 0; j < N; j++)
                    R.e[j] = vec_apply<OP>(A[u].e[j], B[uses::B ? u : 0].e[j], C[uses::C ? u : 0].e[j], k);
                co[i0 + u * VEC_NT] = R;
            }
        }
    }
    // the len % N elements behind the last whole access (at most three), one lane each
    if (N > 1 && blockIdx.x == 0) {
        const size_t i = nchunk * N + t;
        if (t < N - 1 && i < len) {
            const F x = a[i], y = uses::B ? b[i] : x, z = uses::C ? c[i] : x;
            out[i] = vec_apply<OP>(x, y, z, k);
        }
    }
#endif
}

// sppark_poly_product's staging: column j of |dst| (n elements apart) = src_j[0 .. len_j) followed by zeros, both
// columns in one launch (blockIdx.y: the column).  Element-wise: the sources are the caller's, at any element offset.
template<class F>
__global__ __launch_bounds__(VEC_NT)
void k_vec_pad(F* dst, size_t n, const F* src0, size_t len0, const F* src1, size_t len1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr unsigned U = 4;
    const F* src = blockIdx.y ? src1 : src0;
    const size_t len = blockIdx.y ? len1 : len0;
    F* col = dst + (size_t)blockIdx.y * n;
    const size_t step = (size_t)VEC_NT * U, stride = (size_t)gridDim.x * step;
    for (size_t base = (size_t)blockIdx.x * step + threadIdx.x; base < n; base += stride) {
        F x[U];
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = base + u * VEC_NT;
            x[u] = poly_zero<F>();
            if (i < len) x[u] = src[i];
        }
        #pragma unroll
        for (unsigned u = 0; u < U; u++) {
            const size_t i = base + u * VEC_NT;
            if (i < n) col[i] = x[u];
        }
    }
#endif
}

// host side: one launch of k_vec.  |cus|: the device's CU count.  k: |kptr| (a device pointer) when not null, |kval| otherwise.
template<class F, int OP>
static void vec_launch(unsigned cus, F* out, const F* a, const F* b, const F* c, const F& kval, const F* kptr, size_t len, hipStream_t stream)
{
    if (len == 0) return;
    const bool vec = sizeof(F) >= 16 || ((((uintptr_t)out | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0);
    const size_t tiles = (len + vec_geom<F>::T - 1) / vec_geom<F>::T;
    const dim3 grid((unsigned)std::min<size_t>(tiles, (size_t)std::max(cus, 1u) * VEC_WG_PER_CU)), block(VEC_NT);
    auto go = [&](auto VEC, auto KPTR) {
        hipLaunchKernelGGL((k_vec<F, OP, decltype(VEC)::value, decltype(KPTR)::value>), grid, block, 0, stream, out, a, b, c, kval, kptr, len);
    };
    auto with_k = [&](auto VEC) {
        if constexpr (vec_uses<OP>::K) { if (kptr != nullptr) { go(VEC, std::true_type()); return; } }
        go(VEC, std::false_type());
    };
    if constexpr (sizeof(F) < 16) { if (!vec) { with_k(std::false_type()); HIP_OK(hipGetLastError()); return; } }
    with_k(std::true_type());
    HIP_OK(hipGetLastError());
}

} // namespace sppark_amd
