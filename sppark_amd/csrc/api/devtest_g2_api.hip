// Device test hooks for the G2 arithmetic and for every product form of the bucket field, operation by operation
// (exported as sppark_devtest_* from libsppark_<curve>_devtest.so -- a TEST library, never linked into the product ones;
// a translation unit of its own because api/devtest_api.hip already takes the longest to compile).  What the G2 MSM runs
// end to end on random points is run here one operation at a time, on operands the caller chooses: the edges of the
// contracts of ff/montx_blocks.hpp, ff/fp2x_dev.hpp, ec/xyzzx2_dev.hpp and ec/xyzz2_coop.hpp.  tests/test_g2_device_gpu.py.
//
//   a. sppark_devtest_blocks_info / _run : the seven product forms of montx_dev on raw limbs (all five curves)
//   b. sppark_devtest_fp2x_op            : fp2x_dev on internal limbs
//   c. sppark_devtest_fp2_wire_op        : fp2_dev (the loader's type) on wire words
//   d. sppark_devtest_g2_xyzz_op         : one point operation, wire-form XYZZ in and out, by either class
//   e. sppark_devtest_g2_chain           : chains of set / madd steps by the serial class or by wave pairs
// b - e exist on the curves with a G2 only.  Every kernel is built for work-groups of at most 128 lanes.
#include "../msm/curve_select.hpp"
#include "call.hpp"
#if !defined(SPPARK_NO_G2) && !defined(SPPARK_FP2_32LIMB)       // (the A/B build of the old G2 pipeline type has no fp2x_dev)
# define SPPARK_DEVTEST_G2 1
# include "../msm/msm_g2c_kernels.hpp"
#endif
#include <vector>

using namespace sppark_amd;

namespace {
// a device copy of |bytes| host bytes (or an uninitialised buffer when src is null); freed with the scope
struct dev_buf {
    void* p = nullptr;
    dev_buf(const void* src, size_t bytes)
    {
        HIP_OK(hipMalloc(&p, bytes ? bytes : 16));
        if (src && bytes) {
            hipError_t e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) { (void)hipFree(p); p = nullptr; HIP_OK(e); }
        }
    }
    ~dev_buf() { if (p) (void)hipFree(p); }
    dev_buf(const dev_buf&) = delete;
    dev_buf& operator=(const dev_buf&) = delete;
    template<class T> T* as() const { return static_cast<T*>(p); }
};
inline unsigned groups_of_64(size_t n) { return (unsigned)((n + 63) / 64); }
} // namespace

// ---------------------------------------------------------------------------------------------------------------------
// a. The product forms of ff/montx_dev.hpp on raw limbs, one element per lane: the asm statements of ff/montx_blocks.hpp
//    as the device executes them.  Same meaning and numbering as emu_blocks_info / emu_blocks_run of
//    tests/emu/emu_montx_blocks.cpp (which compiles the plain-C bodies of the same blocks for the host).
//    which = 0: the curve's G1 bucket field (msm_fp_d), 1: the base field of its G2 bucket field (fp2_d::fp).
//    form 0: a0 * b0          1: mul2(a0, b0, a1, b1)      2: mul2<true, true>      3: mul2<true, false>
//         4: mul_add          5: sqr2(a0, a1)              6: a0.sqr()
// ---------------------------------------------------------------------------------------------------------------------
template<class F>
__global__ __launch_bounds__(64) void k_blocks_run(u32* r0, u32* r1, const u32* a0, const u32* b0, const u32* a1, const u32* b1,
                                                   unsigned n, int form)
{
    constexpr int NL = F::NL;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * NL;
    const F x0 = F::from_wire(a0 + o), y0 = F::from_wire(b0 + o), x1 = F::from_wire(a1 + o), y1 = F::from_wire(b1 + o);
    F p = F::zero(), q = F::zero();
    switch (form) {
        case 0: p = x0 * y0; break;
        case 1: F::mul2(p, q, x0, y0, x1, y1); break;
        case 2: F::template mul2<true, true>(p, q, x0, y0, x1, y1); break;
        case 3: F::template mul2<true, false>(p, q, x0, y0, x1, y1); break;
        case 4: p = F::mul_add(x0, y0, x1, y1); break;
        case 5: F::sqr2(p, q, x0, x1); break;
        default: p = x0.sqr(); break;
    }
    p.to_wire(r0 + o); q.to_wire(r1 + o);
}

namespace {
template<class F, class P> void blocks_info(int* out)
{
    constexpr int NL = F::NL, LB = F::LIMB_BITS;
    out[0] = NL; out[1] = LB; out[2] = F::FAT_M_OK ? 1 : 0; out[3] = F::MA_A0; out[4] = F::MA_A1; out[5] = F::SQR_L;
    for (int j = 0; j < NL; j++) {                              // limb j of the modulus (montx_dev::mod_limb, on the host)
        const int bit = LB * j, wi = bit >> 5, sh = bit & 31;
        u64 two = wi < (int)P::N ? P::MOD[wi] : 0;
        if (wi + 1 < (int)P::N) two |= (u64)P::MOD[wi + 1] << 32;
        out[8 + j] = (int)((u32)(two >> sh) & ((1u << LB) - 1));
    }
}
template<class F> void blocks_run(int form, void* r0, void* r1, const void* a0, const void* b0, const void* a1, const void* b1, size_t n)
{
    if (form < 0 || form > 6) HIP_OK(hipErrorInvalidValue);
    (void)select_gpu(-1);
    const size_t bytes = n * F::NL * 4;
    dev_buf d_a0(a0, bytes), d_b0(b0, bytes), d_a1(a1, bytes), d_b1(b1, bytes), d_r0(nullptr, bytes), d_r1(nullptr, bytes);
    HIP_OK(hipMemset(d_r0.p, 0, bytes ? bytes : 16)); HIP_OK(hipMemset(d_r1.p, 0, bytes ? bytes : 16));
    if (n) hipLaunchKernelGGL(k_blocks_run<F>, dim3(groups_of_64(n)), dim3(64), 0, 0, d_r0.as<u32>(), d_r1.as<u32>(),
                              d_a0.as<u32>(), d_b0.as<u32>(), d_a1.as<u32>(), d_b1.as<u32>(), (unsigned)n, form);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(r0, d_r0.p, bytes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(r1, d_r1.p, bytes, hipMemcpyDeviceToHost));
}
} // namespace

SPPARK_FFI int sppark_devtest_blocks_info(int which, int* out)
{
    if (which == 0) { blocks_info<msm_fp_d, curve_p::fp>(out); return 0; }
#ifdef SPPARK_DEVTEST_G2
    if (which == 1) { blocks_info<fp2_d::fp, curve_p::fp>(out); return 0; }
#endif
    return -1;
}
SPPARK_FFI RustError sppark_devtest_blocks_run(int which, int form, void* r0, void* r1, const void* a0, const void* b0,
                                               const void* a1, const void* b1, size_t n)
{
    return guarded([&] {
        if (which == 0) { blocks_run<msm_fp_d>(form, r0, r1, a0, b0, a1, b1, n); return; }
#ifdef SPPARK_DEVTEST_G2
        if (which == 1) { blocks_run<fp2_d::fp>(form, r0, r1, a0, b0, a1, b1, n); return; }
#endif
        HIP_OK(hipErrorInvalidValue);
    });
}

#ifdef SPPARK_DEVTEST_G2
typedef xyzz_dev<fp2_wire_d> wire_bucket2_d;
typedef wire_bucket2_d::mem_t wire_bucket2_m;               // the reference's XYZZ image over Fp2: 4 x 2 x fp_d::N words
static_assert(fp2_d::NW == fp2_wire_d::N, "both classes read and write the same wire image");

// ---------------------------------------------------------------------------------------------------------------------
// b. ff/fp2x_dev.hpp on INTERNAL limbs (2 NL words per element, as the caller built them -- non-canonical representatives
//    at the edge of the stated bounds included), as emu_fp2x_op of tests/emu/emu_msm.cpp:
//    op 0: mul<KA>(a, b)   1: a.sqr<KA>()   2: sub<KA>(a, b).norm()   3: neg<KA>(a).norm()      KA in {3, 6, 10, 13}
//       4: (a + b).norm()  6: from_std(first NW words of a)   7: a.to_std() into the first NW words   (ka ignored)
//       5: a.is_zero_mod<KMAX>() into word 0, KMAX = ka in {5, 9, 10, 12}
// ---------------------------------------------------------------------------------------------------------------------
template<int KA>
__global__ __launch_bounds__(64) void k_fp2x_op(u32* out, const u32* a, const u32* b, unsigned n, int op)
{
    typedef fp2_d F;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * F::N;
    const F x = F::from_wire(a + o), y = F::from_wire(b + o);
    F r = F::zero();
    switch (op) {
        case 0: r = F::template mul<KA>(x, y); break;
        case 1: r = x.template sqr<KA>(); break;
        case 2: r = F::template sub<KA>(x, y).norm(); break;
        default: r = F::template neg<KA>(x).norm(); break;
    }
    r.to_wire(out + o);
}
template<int KMAX>
__global__ __launch_bounds__(64) void k_fp2x_is_zero(u32* out, const u32* a, unsigned n)
{
    typedef fp2_d F;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * F::N;
    const F x = F::from_wire(a + o);
    F r = F::zero();
    r.c0.l[0] = x.template is_zero_mod<KMAX>() ? 1u : 0u;
    r.to_wire(out + o);
}
__global__ __launch_bounds__(64) void k_fp2x_misc(u32* out, const u32* a, const u32* b, unsigned n, int op)
{
    typedef fp2_d F;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * F::N;
    u32 w[F::N] = {};
    if (op == 4)      (F::from_wire(a + o) + F::from_wire(b + o)).norm().to_wire(w);
    else if (op == 6) F::from_std(a + o).to_wire(w);
    else              F::from_wire(a + o).to_std(w);
    for (int j = 0; j < F::N; j++) out[o + j] = w[j];
}

SPPARK_FFI RustError sppark_devtest_fp2x_op(int op, int ka, void* out, const void* a, const void* b, size_t n)
{
    return guarded([&] {
        if (op < 0 || op > 7) HIP_OK(hipErrorInvalidValue);
        (void)select_gpu(-1);
        const size_t bytes = n * fp2_d::N * 4;
        dev_buf d_a(a, bytes), d_b(b ? b : a, bytes), d_o(nullptr, bytes);
        const dim3 grid(groups_of_64(n)), block(64);
        u32* o = d_o.as<u32>(); const u32* pa = d_a.as<u32>(); const u32* pb = d_b.as<u32>();
        const unsigned cnt = (unsigned)n;
        if (!n) return;
        if (op == 4 || op >= 6) hipLaunchKernelGGL(k_fp2x_misc, grid, block, 0, 0, o, pa, pb, cnt, op);
        else if (op == 5) {
            if (ka == 5)       hipLaunchKernelGGL(k_fp2x_is_zero<5>, grid, block, 0, 0, o, pa, cnt);
            else if (ka == 9)  hipLaunchKernelGGL(k_fp2x_is_zero<9>, grid, block, 0, 0, o, pa, cnt);
            else if (ka == 10) hipLaunchKernelGGL(k_fp2x_is_zero<10>, grid, block, 0, 0, o, pa, cnt);
            else if (ka == 12) hipLaunchKernelGGL(k_fp2x_is_zero<12>, grid, block, 0, 0, o, pa, cnt);
            else HIP_OK(hipErrorInvalidValue);
        } else {
            if (ka == 3)       hipLaunchKernelGGL(k_fp2x_op<3>, grid, block, 0, 0, o, pa, pb, cnt, op);
            else if (ka == 6)  hipLaunchKernelGGL(k_fp2x_op<6>, grid, block, 0, 0, o, pa, pb, cnt, op);
            else if (ka == 10) hipLaunchKernelGGL(k_fp2x_op<10>, grid, block, 0, 0, o, pa, pb, cnt, op);
            else if (ka == 13) hipLaunchKernelGGL(k_fp2x_op<13>, grid, block, 0, 0, o, pa, pb, cnt, op);
            else HIP_OK(hipErrorInvalidValue);
        }
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out, d_o.p, bytes, hipMemcpyDeviceToHost));
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// c. ff/fp2_dev.hpp over the canonical 32-bit-limb class -- the type the point loader and the wire form use -- on wire
//    words (c0 | c1):  op 0: a + b   1: a - b   2: a * b   3: a.sqr()   4: a.neg()   5: a.dbl()
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_fp2_wire_op(u32* out, const u32* a, const u32* b, unsigned n, int op)
{
    typedef fp2_wire_d F;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)i * F::N;
    const F x = F::from_wire(a + o), y = F::from_wire(b + o);
    F r;
    switch (op) {
        case 0: r = x + y; break;
        case 1: r = x - y; break;
        case 2: r = x * y; break;
        case 3: r = x.sqr(); break;
        case 4: r = x.neg(); break;
        default: r = x.dbl(); break;
    }
    r.to_wire(out + o);
}
SPPARK_FFI RustError sppark_devtest_fp2_wire_op(int op, void* out, const void* a, const void* b, size_t n)
{
    return guarded([&] {
        if (op < 0 || op > 5) HIP_OK(hipErrorInvalidValue);
        (void)select_gpu(-1);
        const size_t bytes = n * fp2_wire_d::N * 4;
        dev_buf d_a(a, bytes), d_b(b ? b : a, bytes), d_o(nullptr, bytes);
        if (!n) return;
        hipLaunchKernelGGL(k_fp2_wire_op, dim3(groups_of_64(n)), dim3(64), 0, 0, d_o.as<u32>(), d_a.as<u32>(), d_b.as<u32>(), (unsigned)n, op);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out, d_o.p, bytes, hipMemcpyDeviceToHost));
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// d. One point operation over Fp2, the XYZZ image in the wire form in and out (X | Y | ZZZ | ZZ, canonical Montgomery
//    words, as store_std writes it; all-zero ZZZ | ZZ = infinity), by F = fp2_wire_d (ec/xyzz_dev.hpp) or F = fp2_d
//    (ec/xyzzx2_dev.hpp, converted with from_std as k_bucket_xyzz_op of api/devtest_api.hip does).
//    op 0: a += b (XYZZ)   1: a += affine(b)   2: a -= affine(b)   3: a = 2a      (b: plain affine points, all-zero = infinity)
// ---------------------------------------------------------------------------------------------------------------------
template<class F>
__global__ __launch_bounds__(64) void k_g2_xyzz_op(wire_bucket2_m* out, const wire_bucket2_m* a, const unsigned char* b, unsigned n, int op)
{
    constexpr int NW = fp2_wire_d::N;
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto load = [](const wire_bucket2_m* src) {
        if constexpr (field_is_internal<F>::value) {
            xyzz_dev<F> r;
            bool inf = true;
            for (int k = 2 * NW; k < 4 * NW; k++) inf &= src->w[k] == 0;
            if (inf) { r.set_inf(); return r; }
            r.X = F::from_std(src->w); r.Y = F::from_std(src->w + NW);
            r.ZZZ = F::from_std(src->w + 2 * NW); r.ZZ = F::from_std(src->w + 3 * NW);
            return r;
        } else {
            return xyzz_dev<F>::load(src);
        }
    };
    xyzz_dev<F> p = load(&a[i]);
    if (op == 0) p.add(load(reinterpret_cast<const wire_bucket2_m*>(b) + i));
    else if (op == 3) p.dbl();
    else {
        const affine_dev<fp2_wire_d> qs = load_affine<fp2_wire_d, false>(b, i, 2 * NW * 4);
        if constexpr (field_is_internal<F>::value) {
            u32 wx[NW], wy[NW];
            qs.X.to_wire(wx); qs.Y.to_wire(wy);
            affine_dev<F> q; q.X = F::from_std(wx); q.Y = F::from_std(wy); q.inf = qs.inf;
            p.madd(q, op == 2);
        } else {
            p.madd(qs, op == 2);
        }
    }
    if constexpr (field_is_internal<F>::value) p.store_std(&out[i]);
    else                                        p.store(&out[i]);
}
SPPARK_FFI RustError sppark_devtest_g2_xyzz_op(int impl, int op, void* out, const void* a, const void* b, size_t n)
{
    return guarded([&] {
        if (op < 0 || op > 3 || impl < 0 || impl > 1) HIP_OK(hipErrorInvalidValue);
        if (!field_is_internal<fp2_d>::value) HIP_OK(hipErrorNotSupported);
        (void)select_gpu(-1);
        const size_t ab = n * sizeof(wire_bucket2_m), bb = op == 3 ? 0 : n * (op == 0 ? sizeof(wire_bucket2_m) : 2 * fp2_wire_d::N * 4);
        dev_buf d_a(a, ab), d_b(op == 3 ? nullptr : b, bb), d_o(nullptr, ab);
        if (!n) return;
        const dim3 grid(groups_of_64(n)), block(64);
        if (impl == 0) hipLaunchKernelGGL(k_g2_xyzz_op<fp2_wire_d>, grid, block, 0, 0, d_o.as<wire_bucket2_m>(), d_a.as<wire_bucket2_m>(), d_b.as<unsigned char>(), (unsigned)n, op);
        else           hipLaunchKernelGGL(k_g2_xyzz_op<fp2_d>, grid, block, 0, 0, d_o.as<wire_bucket2_m>(), d_a.as<wire_bucket2_m>(), d_b.as<unsigned char>(), (unsigned)n, op);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(out, d_o.p, ab, hipMemcpyDeviceToHost));
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// e. Chains of set / madd steps on the product's converted records, the sequence given by the caller (the device form of
//    emu_g2c_chain of tests/emu/emu_msm.cpp): entries[s * nlanes + l] = point index | negate << 31 | restart << 30 is
//    what lane l meets at step s; every lane starts at infinity.  impl 0: the serial class, one lane per chain (set on
//    restart, else madd).  impl 1: g2c_bucket::madd<ROLE> by wave pairs, ceil(nlanes / 64) work-groups of 128, under the
//    contract of ec/xyzz2_coop.hpp: all 128 lanes execute every step and none returns before the last barrier, lanes past
//    the end take the point at infinity, the component is chosen by ONE wave-uniform branch at the kernel's top (as in
//    k_accumulate_g2c).  Both treat a restart on a point at infinity as accumulate_chunk_g2c does: the bucket is emptied.
//    After every step each lane's internal image (X | Y | ZZZ | ZZ, 4 * fp2_d::N words) goes to out[s * nlanes + l].
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_g2_chain_serial(bucket2_m* out, const unsigned char* rec, const u32* entries, unsigned nlanes, unsigned steps)
{
    const unsigned l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nlanes) return;
    bucket2_d acc; acc.set_inf();
    #pragma unroll 1
    for (unsigned s = 0; s < steps; s++) {
        const u32 e = entries[(size_t)s * nlanes + l];
        const affine_dev<fp2_d> pt = load_affine<fp2_d, false>(rec, e & 0x3fffffffu, 0);
        if ((e >> 30) & 1u) acc.set(pt, (e >> 31) != 0);
        else                acc.madd(pt, (e >> 31) != 0);
        acc.store(&out[(size_t)s * nlanes + l]);
    }
}

template<unsigned ROLE>
SPPARK_DEVFN void g2_chain_pair(bucket2_m* out, const unsigned char* rec, const u32* entries, unsigned nlanes, unsigned steps,
                                unsigned l, const g2c_ctx<fp2_d>& c)
{
    const bool act = l < nlanes;
    g2c_bucket<fp2_d> acc; acc.set_inf();
    #pragma unroll 1
    for (unsigned s = 0; s < steps; s++) {              // uniform trip count: barriers inside madd
        u32 e = 0;
        g2c_affine<fp2_d> pt = g2c_affine<fp2_d>::infinity();
        if (act) { e = entries[(size_t)s * nlanes + l]; pt = g2c_affine<fp2_d>::load(rec, e & 0x3fffffffu, ROLE); }
        bool restart = ((e >> 30) & 1u) != 0;
        if (act && pt.inf && restart) { acc.set_inf(); restart = false; }      // (a bucket that starts with the point at infinity)
        acc.template madd<ROLE>(pt, (e >> 31) != 0, restart, c);
        if (act) acc.store(&out[(size_t)s * nlanes + l], ROLE);
    }
}
__global__ __launch_bounds__(128) void k_g2_chain_pairs(bucket2_m* out, const unsigned char* rec, const u32* entries, unsigned nlanes, unsigned steps)
{
    __shared__ g2c_lds<fp2_d> ex;
    const g2c_ctx<fp2_d> c{&ex, threadIdx.x >> 6, threadIdx.x & 63};
    if (c.role == 0) g2_chain_pair<0>(out, rec, entries, nlanes, steps, blockIdx.x * 64 + c.lane, c);
    else             g2_chain_pair<1>(out, rec, entries, nlanes, steps, blockIdx.x * 64 + c.lane, c);
}
__global__ __launch_bounds__(64) void k_g2_internal_to_std(wire_bucket2_m* out, const bucket2_m* in, unsigned n)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) bucket2_d::load(&in[i]).store_std(&out[i]);
}

SPPARK_FFI RustError sppark_devtest_g2_chain(int impl, void* out_internal, void* out_std, const void* points, size_t stride, size_t npoints,
                                             const unsigned* entries, size_t nlanes, unsigned steps)
{
    return guarded([&] {
        typedef affine_loader<fp2_d> AL;
        constexpr size_t PLAIN = 2 * fp2_wire_d::N * 4;
        if (impl < 0 || impl > 1 || (stride != PLAIN && stride != PLAIN + 8) || !npoints || npoints >= (1u << 30) ||
            !nlanes || !steps || nlanes * (size_t)steps >= (1u << 24)) HIP_OK(hipErrorInvalidValue);
        if (!field_is_internal<fp2_d>::value) HIP_OK(hipErrorNotSupported);
        const size_t cnt = nlanes * steps;
        for (size_t k = 0; k < cnt; k++)                            // no entry may point past the records
            if ((entries[k] & 0x3fffffffu) >= npoints) HIP_OK(hipErrorInvalidValue);
        (void)select_gpu(-1);
        dev_buf d_pts(points, npoints * stride), d_rec(nullptr, npoints * AL::STRIDE), d_ent(entries, cnt * 4);
        dev_buf d_out(nullptr, cnt * sizeof(bucket2_m)), d_std(nullptr, cnt * sizeof(wire_bucket2_m));
        const unsigned np = (unsigned)npoints, grid_c = (np + 255) / 256;
        if (stride > PLAIN) hipLaunchKernelGGL((k_convert_points<fp2_d, true>), dim3(grid_c), dim3(256), 0, 0, d_rec.as<unsigned char>(), d_pts.as<unsigned char>(), np, (unsigned)stride);
        else                hipLaunchKernelGGL((k_convert_points<fp2_d, false>), dim3(grid_c), dim3(256), 0, 0, d_rec.as<unsigned char>(), d_pts.as<unsigned char>(), np, (unsigned)stride);
        HIP_OK(hipGetLastError());
        const unsigned groups = groups_of_64(nlanes);
        if (impl == 0) hipLaunchKernelGGL(k_g2_chain_serial, dim3(groups), dim3(64), 0, 0, d_out.as<bucket2_m>(), d_rec.as<unsigned char>(), d_ent.as<u32>(), (unsigned)nlanes, steps);
        else           hipLaunchKernelGGL(k_g2_chain_pairs, dim3(groups), dim3(G2C_NT), 0, 0, d_out.as<bucket2_m>(), d_rec.as<unsigned char>(), d_ent.as<u32>(), (unsigned)nlanes, steps);
        HIP_OK(hipGetLastError());
        if (out_std) {
            hipLaunchKernelGGL(k_g2_internal_to_std, dim3(groups_of_64(cnt)), dim3(64), 0, 0, d_std.as<wire_bucket2_m>(), d_out.as<bucket2_m>(), (unsigned)cnt);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(hipMemcpy(out_internal, d_out.p, cnt * sizeof(bucket2_m), hipMemcpyDeviceToHost));
        if (out_std) HIP_OK(hipMemcpy(out_std, d_std.p, cnt * sizeof(wire_bucket2_m), hipMemcpyDeviceToHost));
    });
}
#endif // SPPARK_DEVTEST_G2
