// The host side of every C entry point: the export macro, the exception barrier, the argument rejections and checked
// size arithmetic, and call_scope -- the one object that owns what a call borrows (staged host buffers, scratch) and
// decides whether the call synchronises.  Host only; exports no symbol; knows no field type.
#pragma once
#include "../util/runtime.hpp"
#include <cstdint>

#define SPPARK_FFI extern "C" __attribute__((visibility("default")))

namespace sppark_amd {

// every entry point's body runs inside this: exceptions become the by-value error of the reference's FFI
template<class Fn> RustError guarded(Fn&& fn)
{
    try { fn(); return rust_ok(); }
    catch (const hip_error& e) { (void)hipGetLastError(); return rust_err(e.code(), e.what()); }
    catch (const std::exception& e) { return rust_err(-1, e.what()); }
    catch (...) { return rust_err(-1, "unknown exception"); }
}

[[noreturn]] inline void reject(const std::string& what)
{   throw hip_error(-(int)hipErrorInvalidValue, what + ": invalid argument");   }

// ---- sizes: a product or sum that does not fit size_t is rejected as |who| + |tail| (built only then) ----
inline size_t checked_mul(size_t a, size_t b, const char* who, const char* tail)
{
    size_t r = 0;
    if (__builtin_mul_overflow(a, b, &r)) reject(std::string(who) + tail);
    return r;
}
inline size_t checked_add(size_t a, size_t b, const char* who, const char* tail)
{
    size_t r = 0;
    if (__builtin_add_overflow(a, b, &r)) reject(std::string(who) + tail);
    return r;
}
// |count| elements of |elem| bytes
inline size_t elems_bytes(size_t count, size_t elem, const char* who, const char* tail = ": len * sizeof(element) overflows size_t")
{   return checked_mul(count, elem, who, tail);   }
// bytes of |batch| >= 1 columns of |n| elements |stride| apart: ((batch - 1) * stride + n) * elem
inline size_t cols_bytes(size_t batch, size_t stride, size_t n, size_t elem, const char* who, const char* tail)
{   return checked_mul(checked_add(checked_mul(batch - 1, stride, who, tail), n, who, tail), elem, who, tail);   }

// [p, p + pb) and [q, q + qb) share a byte
inline bool ranges_meet(const void* p, size_t pb, const void* q, size_t qb)
{
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y ? y - x < pb : x - y < qb;
}
// two buffers of |bytes| bytes must be the same buffer or share no byte
inline void same_or_disjoint(const void* a, const void* b, size_t bytes, const char* what)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    if (x != y && (x < y ? y - x : x - y) < bytes) reject(what);
}

// One per entry-point call.  in / out / inout give the device side of a caller's buffer: a device pointer is itself; a
// host buffer gets a buffer of the scratch pool (util/runtime.hpp), copied in at once and -- out, inout -- copied back by
// finish().  Three rules:
//   1. same host pointer (and size), same device buffer: a pointer staged twice is staged once, and out() of a staged
//      input marks that buffer for the copy back, so identical and in-place arguments stay so on the device;
//   2. finish() enqueues the copies back, synchronises the stream ONCE -- if anything was taken from the pool, if a copy
//      to the host is pending, if the stream is NULL or if the entry point says must_sync -- and only then gives the
//      buffers back to the pool;
//   3. a scope that ends without finish() (an exception) frees its buffers: work that uses them may still be in flight.
// All pointers on the device, no scratch(), a stream: no allocation, no lock, no copy, no synchronisation.
class call_scope {
    struct slot { void* host; void* d; size_t bytes, got, line, lines, pitch; bool back; };     // host == nullptr: scratch
    static constexpr int CAP = 8;       // (the most an entry point borrows is five: sppark_sumcheck_round, 4 tables + scratch)
    slot slots[CAP];
    int used = 0, dev = -1;
    bool to_host = false;
    hipStream_t stream;

    slot& take(void* host, size_t bytes)
    {
        if (used == CAP) reject("call_scope: more buffers than an entry point may borrow");
        if (dev < 0) HIP_OK(hipGetDevice(&dev));
        slot& b = slots[used];
        b = slot{host, nullptr, bytes, 0, bytes, 1, bytes, false};
        b.d = dev_scratch_pool::instance().take(dev, bytes, b.got);
        used++;                          // (from here on the scope owns it, whatever throws)
        return b;
    }
    // |lines| lines of |line| bytes, |pitch| bytes apart on the host and packed on the device
    void* stage(const void* p, size_t line, size_t lines, size_t pitch, bool copy_in, bool back)
    {
        const size_t bytes = line * lines;
        if (bytes == 0) return nullptr;
        if (p == nullptr) HIP_OK(hipErrorInvalidValue);
        for (int i = 0; i < used; i++)
            if (slots[i].host == p && slots[i].bytes == bytes && slots[i].pitch == pitch) { slots[i].back |= back; return slots[i].d; }
        if (is_device_pointer(p)) return (void*)p;
        slot& b = take((void*)p, bytes);
        b.line = line; b.lines = lines; b.pitch = pitch; b.back = back;
        if (copy_in) copy(b, hipMemcpyHostToDevice);
        return b.d;
    }
    void copy(const slot& b, hipMemcpyKind kind)
    {
        const bool in = kind == hipMemcpyHostToDevice;
        if (b.pitch == b.line || b.lines == 1) HIP_OK(hipMemcpyAsync(in ? b.d : b.host, in ? b.host : b.d, b.bytes, kind, stream));
        else HIP_OK(hipMemcpy2DAsync(in ? b.d : b.host, in ? b.line : b.pitch, in ? b.host : b.d, in ? b.pitch : b.line, b.line, b.lines, kind, stream));
    }
public:
    explicit call_scope(hipStream_t s) : stream(s) {}
    call_scope(const call_scope&) = delete;
    ~call_scope() { for (int i = 0; i < used; i++) (void)hipFree(slots[i].d); }

    template<class T> T* in(const void* p, size_t count)  { return (T*)stage(p, count * sizeof(T), 1, count * sizeof(T), true, false); }
    template<class T> T* out(void* p, size_t count)       { return (T*)stage(p, count * sizeof(T), 1, count * sizeof(T), false, true); }
    template<class T> T* inout(void* p, size_t count)     { return (T*)stage(p, count * sizeof(T), 1, count * sizeof(T), true, true); }
    // |lines| lines of |line| elements, |pitch| elements apart.  A device pointer is returned as it is, pitch and all; a host
    // buffer comes back packed (pitch == line), and nothing between its lines is read or written.
    template<class T> T* in_lines(const void* p, size_t line, size_t lines, size_t pitch)
    {   return (T*)stage(p, line * sizeof(T), lines, pitch * sizeof(T), true, false);   }
    template<class T> T* out_lines(void* p, size_t line, size_t lines, size_t pitch)
    {   return (T*)stage(p, line * sizeof(T), lines, pitch * sizeof(T), false, true);   }
    template<class T> T* inout_lines(void* p, size_t line, size_t lines, size_t pitch)
    {   return (T*)stage(p, line * sizeof(T), lines, pitch * sizeof(T), true, true);   }

    // one buffer of the pool for the duration of the call
    void* scratch(size_t bytes) { return take(nullptr, bytes).d; }
    // a result that lies in scratch or in a device buffer and goes to a host pointer: enqueued now, complete after finish()
    void copy_out(void* host, const void* d, size_t bytes)
    {
        HIP_OK(hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, stream));
        to_host = true;
    }
    void finish(bool must_sync = false)
    {
        for (int i = 0; i < used; i++)
            if (slots[i].back) copy(slots[i], hipMemcpyDeviceToHost);
        if (used || to_host || stream == nullptr || must_sync) HIP_OK(hipStreamSynchronize(stream));
        while (used) { used--; dev_scratch_pool::instance().give(dev, slots[used].d, slots[used].got); }
    }
};

} // namespace sppark_amd
