// C entry points of the circle transform over Mersenne31 (include/sppark_amd_circle.h): libsppark_m31 only.
// Every argument is checked before a device is looked up; host buffers are staged through the scratch pool,
// column by column packed, so that nothing between the caller's columns is read or written.
#include "../circle/circle_driver.hpp"

#ifndef FEATURE_MERSENNE31
# error "the circle transform is defined over Mersenne31 only"
#endif

using namespace sppark_amd;
#define SPPARK_FFI extern "C" __attribute__((visibility("default")))

namespace {
template<class Fn> RustError circle_guarded(Fn&& fn)
{
    try { fn(); return rust_ok(); }
    catch (const hip_error& e) { (void)hipGetLastError(); return rust_err(e.code(), e.what()); }
    catch (const std::exception& e) { return rust_err(-1, e.what()); }
    catch (...) { return rust_err(-1, "unknown exception"); }
}
[[noreturn]] void circle_reject(const std::string& what)
{   throw hip_error(-(int)hipErrorInvalidValue, what + ": invalid argument");   }

// bytes of |batch| columns of |n| elements |stride| apart, or a rejection
size_t circle_extent(const char* who, size_t batch, size_t stride, size_t n)
{
    size_t e = 0;
    if (__builtin_mul_overflow(batch - 1, stride, &e) || __builtin_add_overflow(e, n, &e) || __builtin_mul_overflow(e, sizeof(cf_t), &e))
        circle_reject(std::string(who) + ": the extent of the batch overflows size_t");
    return e;
}

// device copy of |batch| host columns, packed (stride n); written back by flush()
struct staged_cols {
    pooled_scratch buf; void* host; size_t n, batch, stride; hipStream_t s;
    staged_cols(void* h, size_t n_, size_t batch_, size_t stride_, hipStream_t s_, bool copy_in)
        : buf(n_ * batch_ * sizeof(cf_t)), host(h), n(n_), batch(batch_), stride(stride_), s(s_)
    {   if (copy_in) HIP_OK(hipMemcpy2DAsync(buf.p, n * sizeof(cf_t), host, stride * sizeof(cf_t), n * sizeof(cf_t), batch, hipMemcpyHostToDevice, s));   }
    cf_t* d() { return (cf_t*)buf.p; }
    void flush()
    {
        HIP_OK(hipMemcpy2DAsync(host, stride * sizeof(cf_t), buf.p, n * sizeof(cf_t), n * sizeof(cf_t), batch, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        buf.done();
    }
};
}

SPPARK_FFI RustError sppark_circle_ntt(size_t device_id, void* inout, uint32_t lg, size_t batch, size_t stride,
                                       int evals_order, int direction, void* stream)
{
    return circle_guarded([&] {
        const char* who = "sppark_circle_ntt";
        if (lg > CIRCLE_MAX_LG) circle_reject(std::string(who) + ": lg above SPPARK_CIRCLE_MAX_LG (30)");
        if (evals_order != CIRCLE_EVALS_BITREV && evals_order != CIRCLE_EVALS_NATURAL) circle_reject(std::string(who) + ": evals_order outside its enum");
        if (direction != CIRCLE_FORWARD && direction != CIRCLE_INVERSE) circle_reject(std::string(who) + ": direction outside its enum");
        const size_t n = (size_t)1 << lg;
        if (stride != 0 && stride < n) circle_reject(std::string(who) + ": 0 < stride < 2^lg");
        if (stride == 0) stride = n;
        if (batch) (void)circle_extent(who, batch, stride, n);
        if (batch == 0 || lg == 0) return;
        if (inout == nullptr) circle_reject(std::string(who) + ": NULL buffer with work to do");
        const gpu_info& gpu = select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        circle_engine& E = circle_engine::instance();
        if (is_device_pointer(inout)) {
            E.run(gpu, (cf_t*)inout, lg, batch, stride, evals_order, direction, s);
            if (s == nullptr) HIP_OK(hipStreamSynchronize(s));          // (a non-NULL stream only enqueues)
            return;
        }
        staged_cols v(inout, n, batch, stride, s, true);
        E.run(gpu, v.d(), lg, batch, n, evals_order, direction, s);
        v.flush();
    });
}

SPPARK_FFI RustError sppark_circle_lde(size_t device_id, void* inout, uint32_t lg, uint32_t lg_blowup, size_t batch,
                                       int evals_order, void* aux_out, void* stream)
{
    return circle_guarded([&] {
        const char* who = "sppark_circle_lde";
        if (lg > CIRCLE_MAX_LG || lg_blowup > CIRCLE_MAX_LG || lg + lg_blowup > CIRCLE_MAX_LG)
            circle_reject(std::string(who) + ": lg + lg_blowup above SPPARK_CIRCLE_MAX_LG (30)");
        if (evals_order != CIRCLE_EVALS_BITREV && evals_order != CIRCLE_EVALS_NATURAL) circle_reject(std::string(who) + ": evals_order outside its enum");
        const size_t dom = (size_t)1 << lg, ext = (size_t)1 << (lg + lg_blowup);
        if (batch) { (void)circle_extent(who, batch, ext, ext); (void)circle_extent(who, batch, dom, dom); }
        if (batch == 0) return;
        if (inout == nullptr) circle_reject(std::string(who) + ": NULL buffer with work to do");
        const gpu_info& gpu = select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        circle_engine& E = circle_engine::instance();
        const bool dev_io = is_device_pointer(inout), dev_aux = aux_out == nullptr || is_device_pointer(aux_out);
        std::unique_ptr<staged_cols> vio, vaux;
        if (!dev_io) vio.reset(new staged_cols(inout, ext, batch, ext, s, true));
        if (!dev_aux) vaux.reset(new staged_cols(aux_out, dom, batch, dom, s, false));
        E.lde(gpu, dev_io ? (cf_t*)inout : vio->d(), lg, lg_blowup, batch, evals_order,
              aux_out == nullptr ? nullptr : (dev_aux ? (cf_t*)aux_out : vaux->d()), s);
        if (vaux) vaux->flush();
        if (vio) vio->flush();
        if ((dev_io && dev_aux) && s == nullptr) HIP_OK(hipStreamSynchronize(s));
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
    return circle_guarded([&] {
        const gpu_info& gpu = select_gpu((int)device_id);
        circle_engine::instance().release(gpu.hip_id);
    });
}
