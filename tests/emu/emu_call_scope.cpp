// CPU harness for csrc/api/call.hpp (tests/test_call_scope.py builds it with the address and undefined-behaviour
// sanitizers and runs it): the HIP runtime entry points that call_scope and the scratch pool use are defined HERE, backed
// by malloc, and count what they are asked to do.  A pointer is a device pointer iff hipMalloc below made it and it has
// not been freed.  One line per case; the first failed expectation ends the program with status 1.
#include "../../sppark_amd/csrc/api/call.hpp"
#include <cstdio>
#include <map>

using namespace sppark_amd;

namespace {
std::map<char*, size_t> live;                   // the fake device's allocations
struct counters { int mallocs, frees, bad_frees, h2d, d2h, copies2d, syncs, d2h_after_sync; } C;
int fail_copy_in = 0;                           // the n-th hipMemcpyAsync from now fails (1: the next one)
int current_device = 0;

bool on_device(const void* p)
{
    auto it = live.upper_bound((char*)p);
    if (it == live.begin()) return false;
    --it;
    return (char*)p < it->first + it->second;
}
void count_copy(hipMemcpyKind kind)
{
    if (kind == hipMemcpyHostToDevice) C.h2d++;
    if (kind == hipMemcpyDeviceToHost) { C.d2h++; if (C.syncs) C.d2h_after_sync++; }
}
void reset() { dev_scratch_pool::instance().release(); C = counters{}; fail_copy_in = 0; }

#define EXPECT(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)
hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x51;        // never dereferenced
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes)
{
    char* q = (char*)malloc(bytes ? bytes : 1);
    memset(q, 0xdd, bytes);
    live[q] = bytes; *p = q; C.mallocs++;
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    if (p == nullptr) return hipSuccess;
    auto it = live.find((char*)p);
    if (it == live.end()) { C.bad_frees++; return hipErrorInvalidValue; }
    live.erase(it); free(p); C.frees++;
    return hipSuccess;
}
hipError_t hipGetDevice(int* d) { *d = current_device; return hipSuccess; }
hipError_t hipSetDevice(int d) { current_device = d; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { C.syncs++; return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    if (fail_copy_in && --fail_copy_in == 0) return hipErrorInvalidValue;
    if (on_device(dst) != (kind == hipMemcpyHostToDevice) || on_device(src) != (kind == hipMemcpyDeviceToHost)) return hipErrorInvalidMemcpyDirection;
    count_copy(kind);
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, hipStream_t)
{
    if (on_device(dst) != (kind == hipMemcpyHostToDevice) || on_device(src) != (kind == hipMemcpyDeviceToHost)) return hipErrorInvalidMemcpyDirection;
    count_copy(kind); C.copies2d++;
    for (size_t r = 0; r < height; r++) memcpy((char*)dst + r * dpitch, (const char*)src + r * spitch, width);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attr, const void* p)
{
    if (!on_device(p)) return hipErrorInvalidValue;             // (what the runtime says of a plain host pointer)
    memset(attr, 0, sizeof(*attr));
    attr->type = hipMemoryTypeDevice;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake runtime error"; }
}

namespace {
uint32_t* dev_alloc(size_t count) { void* p; EXPECT(hipMalloc(&p, count * 4) == hipSuccess); return (uint32_t*)p; }

void all_device()
{
    uint32_t* a = dev_alloc(5); uint32_t* b = dev_alloc(5);
    reset();
    for (hipStream_t s : {STREAM, (hipStream_t)nullptr}) {
        for (bool must : {false, true}) {
            C = counters{};
            call_scope sc(s);
            EXPECT(sc.in<uint32_t>(a, 5) == a && sc.in<uint32_t>(a, 5) == a && sc.out<uint32_t>(b, 5) == b && sc.inout<uint32_t>(a, 5) == a);
            EXPECT(sc.inout_lines<uint32_t>(b, 2, 2, 3) == b);                      // (a device pointer keeps its pitch)
            sc.finish(must);
            EXPECT(C.mallocs == 0 && C.h2d == 0 && C.d2h == 0 && C.copies2d == 0);
            EXPECT(C.syncs == (s == nullptr || must ? 1 : 0));                      // a stream: only enqueued, unless must_sync
        }
    }
    EXPECT(dev_scratch_pool::instance().idle_bytes() == 0);
    (void)hipFree(a); (void)hipFree(b);
    puts("ok all device pointers: no allocation, no copy; one synchronise iff NULL stream or must_sync");
}

void host_in_and_out()
{
    reset();
    uint32_t in[5] = {1, 2, 3, 4, 5}, out[3] = {9, 9, 9};
    {
        call_scope sc(STREAM);
        uint32_t* d_in = sc.in<uint32_t>(in, 5);
        uint32_t* d_out = sc.out<uint32_t>(out, 3);
        EXPECT(d_in != in && d_out != out && d_in != d_out && on_device(d_in) && on_device(d_out));
        EXPECT(C.h2d == 1 && C.d2h == 0 && C.syncs == 0 && C.mallocs == 2);         // the input went over at staging
        for (int i = 0; i < 5; i++) EXPECT(d_in[i] == in[i]);
        for (int i = 0; i < 3; i++) d_out[i] = d_in[i] * 10;                        // "the kernel"
        EXPECT(out[0] == 9);
        sc.finish();
        EXPECT(C.h2d == 1 && C.d2h == 1 && C.syncs == 1 && C.d2h_after_sync == 0);  // the copy back before the one synchronise
    }
    EXPECT(out[0] == 10 && out[1] == 20 && out[2] == 30 && in[4] == 5);
    EXPECT(C.frees == 0 && dev_scratch_pool::instance().idle_bytes() == 5 * 4 + 3 * 4);     // both idle in the pool
    {
        call_scope sc(STREAM);                                                      // the same call again: the pool's buffers
        sc.in<uint32_t>(in, 5); sc.out<uint32_t>(out, 3);
        EXPECT(dev_scratch_pool::instance().idle_bytes() == 0);
        sc.finish();
    }
    EXPECT(C.mallocs == 2 && C.frees == 0 && dev_scratch_pool::instance().idle_bytes() == 32);
    puts("ok host input and output: H2D at staging, D2H in finish() before its one synchronise, buffers pooled and reused");
}

void same_pointer()
{
    reset();
    uint32_t v[4] = {1, 2, 3, 4};
    {
        call_scope sc(STREAM);
        uint32_t* a = sc.in<uint32_t>(v, 4);
        uint32_t* b = sc.in<uint32_t>(v, 4);
        uint32_t* o = sc.out<uint32_t>(v, 4);
        EXPECT(a == b && a == o && C.mallocs == 1 && C.h2d == 1);
        for (int i = 0; i < 4; i++) o[i] = a[i] * b[i];
        sc.finish();
    }
    EXPECT(C.mallocs == 1 && C.h2d == 1 && C.d2h == 1 && C.syncs == 1);
    EXPECT(v[0] == 1 && v[1] == 4 && v[2] == 9 && v[3] == 16);
    {
        call_scope sc(STREAM);                                                      // another size at the same address is another buffer
        uint32_t* a = sc.in<uint32_t>(v, 4);
        uint32_t* o = sc.out<uint32_t>(v, 2);
        EXPECT(a != o);
        o[0] = o[1] = 7;
        sc.finish();
    }
    EXPECT(v[0] == 7 && v[1] == 7 && v[2] == 9 && v[3] == 16);
    puts("ok one host pointer as two inputs and the output: one buffer, one H2D, one D2H");
}

void strided_lines()
{
    reset();
    const uint32_t GAP = 0xabababab;
    uint32_t m[3 * 4], ro[2 * 5];                                                   // 3 lines of 2, pitch 4; 2 lines of 3, pitch 5
    for (int i = 0; i < 12; i++) m[i] = i % 4 < 2 ? 100 + i : GAP;
    for (int i = 0; i < 10; i++) ro[i] = i % 5 < 3 ? 200 + i : GAP;
    {
        call_scope sc(STREAM);
        uint32_t* d = sc.inout_lines<uint32_t>(m, 2, 3, 4);
        const uint32_t* r = sc.in_lines<uint32_t>(ro, 3, 2, 5);
        EXPECT(C.copies2d == 2 && C.h2d == 2);
        for (int l = 0; l < 3; l++) for (int i = 0; i < 2; i++) EXPECT(d[l * 2 + i] == 100u + l * 4 + i);      // packed: only the elements
        for (int l = 0; l < 2; l++) for (int i = 0; i < 3; i++) EXPECT(r[l * 3 + i] == 200u + l * 5 + i);
        for (int i = 0; i < 6; i++) d[i] += 1000;
        sc.finish();
        EXPECT(C.d2h == 1 && C.copies2d == 3 && C.syncs == 1);
    }
    for (int i = 0; i < 12; i++) EXPECT(m[i] == (i % 4 < 2 ? 1100u + i : GAP));     // the gaps are as they were
    for (int i = 0; i < 10; i++) EXPECT(ro[i] == (i % 5 < 3 ? 200u + i : GAP));
    EXPECT(dev_scratch_pool::instance().idle_bytes() == 6 * 4 + 6 * 4);
    {
        call_scope sc(STREAM);                                                      // pitch == line: one plain copy each way
        C = counters{};
        uint32_t* d = sc.inout_lines<uint32_t>(m, 4, 3, 4);
        EXPECT(C.copies2d == 0 && C.h2d == 1 && d[5] == 1105);
        sc.finish();
        EXPECT(C.copies2d == 0 && C.d2h == 1);
    }
    puts("ok strided lines: packed on the device, the gaps of the host buffer neither read nor written");
}

void scratch_and_must_sync()
{
    reset();
    {
        call_scope sc(STREAM);
        void* p = sc.scratch(64);
        EXPECT(on_device(p) && C.mallocs == 1 && C.h2d == 0);
        sc.finish();
        EXPECT(C.syncs == 1 && C.d2h == 0);
    }
    EXPECT(C.frees == 0 && dev_scratch_pool::instance().idle_bytes() == 64);
    uint32_t* d = dev_alloc(2);
    d[0] = 5; d[1] = 6;
    C = counters{};
    uint32_t host[2] = {0, 0};
    {
        call_scope sc(STREAM);                                                      // a device result that goes to a host pointer
        sc.copy_out(host, d, 8);
        sc.finish();
        EXPECT(C.d2h == 1 && C.syncs == 1 && C.d2h_after_sync == 0 && C.mallocs == 0);
    }
    EXPECT(host[0] == 5 && host[1] == 6);
    (void)hipFree(d);
    puts("ok scratch() alone and copy_out() alone each make finish() synchronise once; the scratch goes back to the pool");
}

void failing_copy()
{
    reset();
    uint32_t a[4] = {1, 2, 3, 4}, b[4] = {5, 6, 7, 8};
    const size_t live_before = live.size();
    bool thrown = false;
    try {
        call_scope sc(STREAM);
        sc.in<uint32_t>(a, 4);
        sc.scratch(32);
        fail_copy_in = 1;
        sc.in<uint32_t>(b, 4);                                                      // its buffer is taken, then the copy fails
        EXPECT(!"the failed copy did not throw");
    } catch (const hip_error& e) { thrown = e.code() == -(int)hipErrorInvalidValue; }
    EXPECT(thrown);
    EXPECT(C.mallocs == 3 && C.frees == 3 && C.bad_frees == 0 && live.size() == live_before);      // freed, all three, once each
    EXPECT(dev_scratch_pool::instance().idle_bytes() == 0 && C.syncs == 0);                          // and never pooled

    reset();
    thrown = false;
    try {
        call_scope sc(STREAM);
        sc.inout<uint32_t>(a, 4);
        sc.out<uint32_t>(b, 4);
        fail_copy_in = 2;                                                           // the second copy back, inside finish()
        sc.finish();
        EXPECT(!"the failed copy did not throw");
    } catch (const hip_error&) { thrown = true; }
    EXPECT(thrown && C.mallocs == 2 && C.frees == 2 && C.bad_frees == 0 && C.syncs == 0 && live.size() == live_before);
    EXPECT(dev_scratch_pool::instance().idle_bytes() == 0);
    puts("ok a failing copy: the exception propagates, every buffer of the scope is freed once, none is pooled");
}

template<class Fn> bool rejected(Fn&& fn, const char* text)
{
    try { fn(); return false; }
    catch (const hip_error& e) { return e.code() == -(int)hipErrorInvalidValue && std::string(e.what()) == text; }
}

void size_helpers()
{
    const size_t MAX = SIZE_MAX;
    EXPECT(checked_mul(MAX, 1, "f", ": t") == MAX && checked_mul(MAX / 5, 5, "f", ": t") == MAX && checked_mul(0, MAX, "f", ": t") == 0);
    EXPECT(rejected([&] { checked_mul(MAX / 2 + 1, 2, "f", ": t"); }, "f: t: invalid argument"));
    EXPECT(checked_add(MAX - 1, 1, "f", ": t") == MAX);
    EXPECT(rejected([&] { checked_add(MAX, 1, "f", ": t"); }, "f: t: invalid argument"));
    EXPECT(elems_bytes(MAX / 8, 8, "f") == MAX - 7);
    EXPECT(rejected([&] { elems_bytes(MAX / 8 + 1, 8, "f"); }, "f: len * sizeof(element) overflows size_t: invalid argument"));
    EXPECT(cols_bytes(1, 0, 7, 4, "f", ": e") == 28 && cols_bytes(3, 10, 7, 4, "f", ": e") == 108);
    EXPECT(cols_bytes(2, MAX - 1, 1, 1, "f", ": e") == MAX && cols_bytes(2, MAX / 5 - 1, 1, 5, "f", ": e") == MAX);     // (SIZE_MAX is a multiple of 5)
    EXPECT(rejected([&] { cols_bytes(3, MAX / 2 + 1, 1, 1, "f", ": e"); }, "f: e: invalid argument"));     // the product
    EXPECT(rejected([&] { cols_bytes(2, MAX - 1, 2, 1, "f", ": e"); }, "f: e: invalid argument"));         // the sum
    EXPECT(rejected([&] { cols_bytes(2, MAX - 1, 1, 2, "f", ": e"); }, "f: e: invalid argument"));         // the element size
    EXPECT(rejected([&] { reject("who: what"); }, "who: what: invalid argument"));

    char buf[16];
    EXPECT(!ranges_meet(buf, 4, buf + 4, 4) && !ranges_meet(buf + 4, 4, buf, 4));   // touching, no byte shared
    EXPECT(ranges_meet(buf, 4, buf + 3, 4) && ranges_meet(buf + 3, 4, buf, 4));     // one byte shared, either order
    EXPECT(ranges_meet(buf, 8, buf + 2, 1) && ranges_meet(buf + 2, 1, buf, 8) && ranges_meet(buf, 4, buf, 4));
    same_or_disjoint(buf, buf, 8, "x");                                             // identical: accepted
    same_or_disjoint(buf, buf + 8, 8, "x"); same_or_disjoint(buf + 8, buf, 8, "x");
    EXPECT(rejected([&] { same_or_disjoint(buf, buf + 7, 8, "x"); }, "x: invalid argument"));
    EXPECT(rejected([&] { same_or_disjoint(buf + 1, buf, 8, "x"); }, "x: invalid argument"));
    puts("ok size helpers: SIZE_MAX passes, one more is rejected with the caller's text; ranges and pairs");
}
}

int main()
{
    all_device();
    host_in_and_out();
    same_pointer();
    strided_lines();
    scratch_and_must_sync();
    failing_copy();
    size_helpers();
    reset();
    EXPECT(live.empty() && C.bad_frees == 0);                   // nothing of the fake device is left
    puts("ok nothing left allocated");
    return 0;
}
