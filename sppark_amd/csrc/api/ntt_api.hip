// C-ABI of the NTT library (one .so per field: -DFEATURE_GOLDILOCKS /
// -DFEATURE_BABY_BEAR, as poc/ntt-cuda/build.rs selects them).  Declarations +
// reference citations: include/sppark_amd.h.
#include "../ntt/field_select.hpp"
namespace sppark_amd {
#define SPPARK_NTT_EXTERN(DIF, INV, R1, R2) \
    extern template __global__ void k_ntt_pass<ntt_fr_t, DIF, INV, R1, R2>(ntt_fr_t*, ntt_tables<ntt_fr_t>, ntt_pass, size_t);
SPPARK_NTT_PASS_ALL(SPPARK_NTT_EXTERN, true) SPPARK_NTT_PASS_ALL(SPPARK_NTT_EXTERN, false)
#define SPPARK_NTT_SMALL_EXTERN(INV, LGC) \
    extern template __global__ void k_ntt_small<ntt_fr_t, INV, LGC>(ntt_fr_t*, ntt_tables<ntt_fr_t>, ntt_tables<ntt_fr_t>, unsigned, size_t);
#define SPPARK_NTT_PACKED_EXTERN(INV, LG) \
    extern template __global__ void k_ntt_small_packed<ntt_fr_t, INV, LG>(ntt_fr_t*, ntt_tables<ntt_fr_t>, ntt_tables<ntt_fr_t>, unsigned, size_t, size_t);
SPPARK_NTT_PACKED_ALL(SPPARK_NTT_PACKED_EXTERN)
#if defined(FEATURE_GOLDILOCKS) || defined(FEATURE_BABY_BEAR)
SPPARK_NTT_SMALL_ALL_NARROW(SPPARK_NTT_SMALL_EXTERN)
#else
SPPARK_NTT_SMALL_ALL_WIDE(SPPARK_NTT_SMALL_EXTERN)
#endif
#if defined(FEATURE_GOLDILOCKS) || defined(FEATURE_BABY_BEAR)
SPPARK_NTT_PASS_ALL_BIG(SPPARK_NTT_EXTERN, true) SPPARK_NTT_PASS_ALL_BIG(SPPARK_NTT_EXTERN, false)
#else
#define SPPARK_NTT_LAT_EXTERN(DIF, INV) \
    extern template __global__ void k_ntt_pass_lat<ntt_fr_t, DIF, INV>(ntt_fr_t*, ntt_tables<ntt_fr_t>, ntt_pass, size_t);
SPPARK_NTT_LAT_EXTERN(true, false) SPPARK_NTT_LAT_EXTERN(true, true) SPPARK_NTT_LAT_EXTERN(false, false) SPPARK_NTT_LAT_EXTERN(false, true)
#endif
}
#if defined(FEATURE_GOLDILOCKS) || defined(FEATURE_BABY_BEAR)      // the radix-64 plan: ntt/k_ntt_r64.hip
#include "../ntt/ntt_r64_kernels.hpp"
namespace sppark_amd {
#define SPPARK_R64_EXTERN(K, DIF, INV) \
    extern template __global__ void K<ntt_fr_t, DIF, INV>(ntt_fr_t*, ntt_r64_args<ntt_fr_t>, size_t);
SPPARK_R64_EXTERN(k_ntt6, true, false) SPPARK_R64_EXTERN(k_ntt6, true, true) SPPARK_R64_EXTERN(k_ntt6, false, false) SPPARK_R64_EXTERN(k_ntt6, false, true)
SPPARK_R64_EXTERN(k_ntt12, true, false) SPPARK_R64_EXTERN(k_ntt12, true, true) SPPARK_R64_EXTERN(k_ntt12, false, false) SPPARK_R64_EXTERN(k_ntt12, false, true)
extern template __global__ void k_ntt12<ntt_fr_t, false, false, true>(ntt_fr_t*, ntt_r64_args<ntt_fr_t>, size_t);
}
#endif
#include "../ntt/ntt_driver.hpp"
#ifdef SPPARK_NTT_WITH_MSM            // same .so as msm_api.hip, which already defines the common symbols
# include "call.hpp"
#else
# include "common_api.hpp"
#endif

using namespace sppark_amd;
typedef ntt_fr_t fr_t;

static void ntt_any(size_t device_id, void* inout, uint32_t lg, int order, int direction, int type, hipStream_t stream)
{
    if (lg == 0) return;
    // the arguments are checked before anything is allocated or copied: the size is only meaningful (and the caller's
    // buffer only that large) for an lg the field accepts
    if (lg > fr_t::TWO_ADICITY || order < 0 || order > 3) HIP_OK(hipErrorInvalidValue);
    const gpu_info& gpu = select_gpu((int)device_id);
    // a host buffer: H2D, transform, D2H (NTT::Base, ntt/ntt.cuh:216-244); a device buffer and a stream: only enqueued
    call_scope sc(stream);
    fr_t* d = sc.inout<fr_t>(inout, (size_t)1 << lg);
    ntt_engine<fr_t>::instance().run(gpu, d, lg, order, direction, type, stream);
    sc.finish();
}

SPPARK_FFI RustError compute_ntt(size_t device_id, void* inout, uint32_t lg_domain_size,
                                 int ntt_order, int ntt_direction, int ntt_type)
{   return guarded([&] { ntt_any(device_id, inout, lg_domain_size, ntt_order, ntt_direction, ntt_type, nullptr); });   }

SPPARK_FFI RustError sppark_ntt(size_t device_id, void* inout, uint32_t lg_domain_size,
                                int ntt_order, int ntt_direction, int ntt_type, void* stream)
{   return guarded([&] { ntt_any(device_id, inout, lg_domain_size, ntt_order, ntt_direction, ntt_type, (hipStream_t)stream); });   }

// ---- low-degree extension (C++-only in the reference: NTT::LDE / LDE_aux / LDE_powers / LDE_expand) ----
static void lde_any(size_t device_id, void* inout, uint32_t lg_domain, uint32_t lg_blowup, void* aux_out, hipStream_t stream)
{
    if ((uint64_t)lg_domain + lg_blowup > fr_t::TWO_ADICITY) HIP_OK(hipErrorInvalidValue);     // (before the scratch and the copies)
    const gpu_info& gpu = select_gpu((int)device_id);
    const size_t dom = (size_t)1 << lg_domain, ext = dom << lg_blowup;
    const bool dev = is_device_pointer(inout), aux_dev = aux_out && is_device_pointer(aux_out);
    // scratch: [tmp: dom][aux: dom, when it has to be staged][ext, when inout is a host buffer]
    // (one buffer, and of inout only the 2^lg_domain evaluations go to the device: the scope's scratch, not its staging)
    const size_t need = dom + (aux_out && !aux_dev ? dom : 0) + (dev ? 0 : ext);
    call_scope sc(stream);
    fr_t* scratch = (fr_t*)sc.scratch(need * sizeof(fr_t));
    fr_t* d_tmp = scratch;
    fr_t* d_aux = aux_out ? (aux_dev ? (fr_t*)aux_out : scratch + dom) : nullptr;
    fr_t* d_ext = dev ? (fr_t*)inout : scratch + need - ext;
    if (!dev) HIP_OK(hipMemcpyAsync(d_ext, inout, dom * sizeof(fr_t), hipMemcpyHostToDevice, stream));
    ntt_engine<fr_t>::instance().lde(gpu, d_ext, d_tmp, d_aux, lg_domain, lg_blowup, stream);
    if (aux_out && !aux_dev) sc.copy_out(aux_out, d_aux, dom * sizeof(fr_t));
    if (!dev) sc.copy_out(inout, d_ext, ext * sizeof(fr_t));
    sc.finish();
}
SPPARK_FFI void sppark_ntt_release_cached(void)
{
    dev_scratch_pool::instance().release();
    ntt_engine<fr_t>::instance().release_tables();
}
// diagnostics for the tests: idle scratch bytes of this library's pool, cached twiddle tables
SPPARK_FFI size_t sppark_ntt_cached_scratch_bytes(void) { return dev_scratch_pool::instance().idle_bytes(); }
SPPARK_FFI size_t sppark_ntt_cached_tables(void) { return ntt_engine<fr_t>::instance().cached_table_count(); }

SPPARK_FFI RustError sppark_lde(size_t device_id, void* inout, uint32_t lg_domain_size, uint32_t lg_blowup,
                                void* aux_out, void* stream)
{   return guarded([&] { lde_any(device_id, inout, lg_domain_size, lg_blowup, aux_out, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_lde_powers(size_t device_id, void* d_inout, uint32_t lg_domain_size, void* stream)
{
    return guarded([&] {
        if (!is_device_pointer(d_inout)) HIP_OK(hipErrorInvalidValue);
        ntt_engine<fr_t>::instance().lde_powers(select_gpu((int)device_id), (fr_t*)d_inout, lg_domain_size, (hipStream_t)stream);
        if (stream == nullptr) HIP_OK(hipStreamSynchronize(nullptr));
    });
}

SPPARK_FFI RustError sppark_lde_expand(size_t device_id, void* d_out, const void* d_in, uint32_t lg_domain_size,
                                       uint32_t lg_blowup, void* stream)
{
    return guarded([&] {
        if (!is_device_pointer(d_out) || !is_device_pointer(d_in)) HIP_OK(hipErrorInvalidValue);
        ntt_engine<fr_t>::instance().lde_spread(select_gpu((int)device_id), (fr_t*)d_out, (const fr_t*)d_in,
                                                lg_domain_size, lg_blowup, false, (hipStream_t)stream);
        if (stream == nullptr) HIP_OK(hipStreamSynchronize(nullptr));
    });
}

// ---- batched transforms (include/sppark_amd_batch.h) ----
static constexpr size_t BATCH_CHUNK_BYTES = (size_t)256 << 20;    // SPPARK_BATCH_CHUNK_BYTES

// a device buffer's extent must lie inside the allocation that holds its first byte
static void check_device_extent(const void* p, size_t bytes, const char* what)
{
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); reject(what); }
    const size_t off = (size_t)((const char*)p - (const char*)base);
    if (off > size || bytes > size - off) reject(what);
}

static void ntt_batch_any(size_t device_id, void* inout, uint32_t lg, size_t batch, size_t stride, int order, int direction, int type,
                          hipStream_t stream)
{
    if (lg > fr_t::TWO_ADICITY) reject("sppark_ntt_batch: lg_domain_size above the field's 2-adicity");
    if (order < 0 || order > 3) reject("sppark_ntt_batch: ntt_order outside 0..3");
    const size_t n = (size_t)1 << lg;
    if (stride == 0) stride = n;
    if (stride < n) reject("sppark_ntt_batch: stride below 2^lg_domain_size");
    if (batch == 0 || lg == 0) return;
    const size_t bytes = cols_bytes(batch, stride, n, sizeof(fr_t), "sppark_ntt_batch", ": extent overflows size_t");
    const gpu_info& gpu = select_gpu((int)device_id);
    auto& E = ntt_engine<fr_t>::instance();
    if (is_device_pointer(inout)) {
        check_device_extent(inout, bytes, "sppark_ntt_batch: inout extends past its allocation");
        E.run(gpu, (fr_t*)inout, lg, order, direction, type, stream, nullptr, batch, stride);
        if (stream == nullptr) HIP_OK(hipStreamSynchronize(stream));
        return;
    }
    // host buffer: chunks of whole columns through one packed device buffer (the gaps between columns are never copied)
    const size_t col = n * sizeof(fr_t), cols = std::min(batch, std::max<size_t>(1, BATCH_CHUNK_BYTES / col));
    call_scope sc(stream);
    fr_t* d = (fr_t*)sc.scratch(cols * col);
    for (size_t c0 = 0; c0 < batch; c0 += cols) {
        const size_t k = std::min(cols, batch - c0);
        char* h = (char*)inout + c0 * stride * sizeof(fr_t);
        if (stride == n) HIP_OK(hipMemcpyAsync(d, h, k * col, hipMemcpyHostToDevice, stream));
        else HIP_OK(hipMemcpy2DAsync(d, col, h, stride * sizeof(fr_t), col, k, hipMemcpyHostToDevice, stream));
        E.run(gpu, d, lg, order, direction, type, stream, nullptr, k, n);
        if (stride == n) HIP_OK(hipMemcpyAsync(h, d, k * col, hipMemcpyDeviceToHost, stream));
        else HIP_OK(hipMemcpy2DAsync(h, stride * sizeof(fr_t), d, col, col, k, hipMemcpyDeviceToHost, stream));
    }
    sc.finish();
}

static void lde_batch_any(size_t device_id, void* inout, uint32_t lg_domain, uint32_t lg_blowup, size_t batch, void* aux_out,
                          hipStream_t stream)
{
    if ((uint64_t)lg_domain + lg_blowup > fr_t::TWO_ADICITY) reject("sppark_lde_batch: lg_domain_size + lg_blowup above the field's 2-adicity");
    const size_t dom = (size_t)1 << lg_domain, ext = dom << lg_blowup;
    if (batch == 0) return;
    const size_t ext_bytes = cols_bytes(batch, ext, ext, sizeof(fr_t), "sppark_lde_batch", ": extent overflows size_t");
    const size_t aux_bytes = cols_bytes(batch, dom, dom, sizeof(fr_t), "sppark_lde_batch", ": aux_out extent overflows size_t");
    const gpu_info& gpu = select_gpu((int)device_id);
    const bool dev = is_device_pointer(inout), aux_dev = aux_out && is_device_pointer(aux_out);
    if (dev) check_device_extent(inout, ext_bytes, "sppark_lde_batch: inout extends past its allocation");
    if (aux_dev) check_device_extent(aux_out, aux_bytes, "sppark_lde_batch: aux_out extends past its allocation");
    // device scratch per column: [tmp: dom][aux: dom, when it has to be staged][ext, when inout is a host buffer]; whole
    // columns per chunk, SPPARK_BATCH_CHUNK_BYTES at most (one column when a column needs more)
    const size_t per_col = (dom + (aux_out && !aux_dev ? dom : 0) + (dev ? 0 : ext)) * sizeof(fr_t);
    const size_t cols = std::min(batch, std::max<size_t>(1, BATCH_CHUNK_BYTES / per_col));
    call_scope sc(stream);
    fr_t* d_tmp = (fr_t*)sc.scratch(cols * per_col);
    fr_t* d_stage_aux = d_tmp + cols * dom;
    fr_t* d_stage_ext = d_stage_aux + (aux_out && !aux_dev ? cols * dom : 0);
    auto& E = ntt_engine<fr_t>::instance();
    for (size_t c0 = 0; c0 < batch; c0 += cols) {
        const size_t k = std::min(cols, batch - c0);
        fr_t* h_ext = (fr_t*)inout + c0 * ext;
        fr_t* d_ext = dev ? h_ext : d_stage_ext;
        fr_t* d_aux = aux_out ? (aux_dev ? (fr_t*)aux_out + c0 * dom : d_stage_aux) : nullptr;
        if (!dev) HIP_OK(hipMemcpy2DAsync(d_ext, ext * sizeof(fr_t), h_ext, ext * sizeof(fr_t), dom * sizeof(fr_t), k, hipMemcpyHostToDevice, stream));
        E.lde(gpu, d_ext, d_tmp, d_aux, lg_domain, lg_blowup, stream, k);
        if (aux_out && !aux_dev) HIP_OK(hipMemcpyAsync((fr_t*)aux_out + c0 * dom, d_aux, k * dom * sizeof(fr_t), hipMemcpyDeviceToHost, stream));
        if (!dev) HIP_OK(hipMemcpyAsync(h_ext, d_ext, k * ext * sizeof(fr_t), hipMemcpyDeviceToHost, stream));
    }
    sc.finish();
}

SPPARK_FFI RustError sppark_ntt_batch(size_t device_id, void* inout, uint32_t lg_domain_size, size_t batch, size_t stride,
                                      int ntt_order, int ntt_direction, int ntt_type, void* stream)
{   return guarded([&] { ntt_batch_any(device_id, inout, lg_domain_size, batch, stride, ntt_order, ntt_direction, ntt_type, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_lde_batch(size_t device_id, void* inout, uint32_t lg_domain_size, uint32_t lg_blowup, size_t batch,
                                      void* aux_out, void* stream)
{   return guarded([&] { lde_batch_any(device_id, inout, lg_domain_size, lg_blowup, batch, aux_out, (hipStream_t)stream); });   }

SPPARK_FFI size_t sppark_ntt_batch_launch_cols(size_t device_id, uint32_t lg_domain_size)
{
    if (lg_domain_size > fr_t::TWO_ADICITY) return 0;
    try { return ntt_engine<fr_t>::instance().launch_cols(select_gpu((int)device_id), lg_domain_size); }
    catch (...) { (void)hipGetLastError(); return 0; }
}

#include "poly_api.hpp"
#include "field_api.hpp"
#define SPPARK_VEC_WITH_NTT 1       // sppark_poly_product, sppark_poly_vanishing_quotient
#include "vec_api.hpp"
#include "mle_api.hpp"
#include "merkle_api.hpp"
#include "fri_api.hpp"
#if defined(FEATURE_GOLDILOCKS) || defined(FEATURE_BABY_BEAR)      // the fields Poseidon2 is defined over here
# include "poseidon2_api.hpp"
#endif
