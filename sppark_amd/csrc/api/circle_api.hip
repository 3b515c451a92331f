// C entry points of the circle transform over Mersenne31 (include/sppark_amd_circle.h): libsppark_m31 only.
// Every argument is checked before a device is looked up; host buffers are staged by a call_scope (api/call.hpp),
// column by column packed, so that nothing between the caller's columns is read or written.
#include "../circle/circle_driver.hpp"
#include "call.hpp"

#ifndef FEATURE_MERSENNE31
# error "the circle transform is defined over Mersenne31 only"
#endif

using namespace sppark_amd;

namespace {
constexpr const char* CIRCLE_OVERFLOW = ": the extent of the batch overflows size_t";
}

SPPARK_FFI RustError sppark_circle_ntt(size_t device_id, void* inout, uint32_t lg, size_t batch, size_t stride,
                                       int evals_order, int direction, void* stream)
{
    return guarded([&] {
        const char* who = "sppark_circle_ntt";
        if (lg > CIRCLE_MAX_LG) reject(std::string(who) + ": lg above SPPARK_CIRCLE_MAX_LG (30)");
        if (evals_order != CIRCLE_EVALS_BITREV && evals_order != CIRCLE_EVALS_NATURAL) reject(std::string(who) + ": evals_order outside its enum");
        if (direction != CIRCLE_FORWARD && direction != CIRCLE_INVERSE) reject(std::string(who) + ": direction outside its enum");
        const size_t n = (size_t)1 << lg;
        if (stride != 0 && stride < n) reject(std::string(who) + ": 0 < stride < 2^lg");
        if (stride == 0) stride = n;
        if (batch) (void)cols_bytes(batch, stride, n, sizeof(cf_t), who, CIRCLE_OVERFLOW);
        if (batch == 0 || lg == 0) return;
        if (inout == nullptr) reject(std::string(who) + ": NULL buffer with work to do");
        const gpu_info& gpu = select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        call_scope sc(s);
        cf_t* d = sc.inout_lines<cf_t>(inout, n, batch, stride);
        circle_engine::instance().run(gpu, d, lg, batch, d == inout ? stride : n, evals_order, direction, s);   // (a host buffer comes packed)
        sc.finish();                                                    // (device columns and a stream: only enqueued)
    });
}

SPPARK_FFI RustError sppark_circle_lde(size_t device_id, void* inout, uint32_t lg, uint32_t lg_blowup, size_t batch,
                                       int evals_order, void* aux_out, void* stream)
{
    return guarded([&] {
        const char* who = "sppark_circle_lde";
        if (lg > CIRCLE_MAX_LG || lg_blowup > CIRCLE_MAX_LG || lg + lg_blowup > CIRCLE_MAX_LG)
            reject(std::string(who) + ": lg + lg_blowup above SPPARK_CIRCLE_MAX_LG (30)");
        if (evals_order != CIRCLE_EVALS_BITREV && evals_order != CIRCLE_EVALS_NATURAL) reject(std::string(who) + ": evals_order outside its enum");
        const size_t dom = (size_t)1 << lg, ext = (size_t)1 << (lg + lg_blowup);
        if (batch) { (void)cols_bytes(batch, ext, ext, sizeof(cf_t), who, CIRCLE_OVERFLOW); (void)cols_bytes(batch, dom, dom, sizeof(cf_t), who, CIRCLE_OVERFLOW); }
        if (batch == 0) return;
        if (inout == nullptr) reject(std::string(who) + ": NULL buffer with work to do");
        const gpu_info& gpu = select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        call_scope sc(s);
        cf_t* d_io = sc.inout<cf_t>(inout, batch * ext);
        cf_t* d_aux = aux_out == nullptr ? nullptr : sc.out<cf_t>(aux_out, batch * dom);
        circle_engine::instance().lde(gpu, d_io, lg, lg_blowup, batch, evals_order, d_aux, s);
        sc.finish();
    });
}

// bytes of the tables kept for this device (the point tables and the inverse twiddles up to 2^24: at most
// SPPARK_CIRCLE_CACHE_CAP_BYTES); 0 without a device
SPPARK_FFI size_t sppark_circle_cached_bytes(size_t device_id)
{
    try {
        auto& gpus = gpus_t::all();
        if (device_id >= gpus.size()) return 0;
        return circle_engine::instance().cached_bytes(gpus[device_id].hip_id);
    } catch (...) { return 0; }
}

SPPARK_FFI RustError sppark_circle_release_cached(size_t device_id)
{
    return guarded([&] {
        const gpu_info& gpu = select_gpu((int)device_id);
        circle_engine::instance().release(gpu.hip_id);
    });
}
