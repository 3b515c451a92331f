// C entry points of the field-vector inverse and quotient over the library's field fr_t
// (include/sppark_amd_field.h; the reference's ff/batch_inversion.hpp is a host-side C++ template).
// Included next to api/poly_api.hpp, whose dev_view stages host buffers.
// Expects: fr_t, guarded(), SPPARK_FFI, select_gpu, is_device_pointer in scope.
#pragma once
#include "poly_api.hpp"

namespace {
[[noreturn]] void field_reject(const char* what)
{   throw hip_error(-(int)hipErrorInvalidValue, std::string(what) + ": invalid argument");   }

// two buffers of |bytes| bytes must be the same buffer or share no byte
void field_check_pair(const void* a, const void* b, size_t bytes, const char* what)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    if (x != y && (x < y ? y - x : x - y) < bytes) field_reject(what);
}

// out[i] = num[i] / den[i] (num == nullptr: 1 / den[i]); every argument is checked before a device is looked up
void field_inverse_any(const char* name, size_t device_id, void* out, const void* num, bool divide, const void* den, size_t len, hipStream_t s)
{
    if (len == 0) return;
    const std::string who(name);
    if (out == nullptr || den == nullptr || (divide && num == nullptr)) field_reject((who + ": NULL buffer with len > 0").c_str());
    size_t bytes = 0;
    if (__builtin_mul_overflow(len, sizeof(fr_t), &bytes)) field_reject((who + ": len * sizeof(element) overflows size_t").c_str());
    const std::string lap = who + ": buffers overlap partially (any two must be identical or disjoint)";
    field_check_pair(out, den, bytes, lap.c_str());
    if (divide) { field_check_pair(out, num, bytes, lap.c_str()); field_check_pair(num, den, bytes, lap.c_str()); }
    (void)select_gpu((int)device_id);

    dev_view vden(den, len, true, s);
    dev_view vnum(divide && num != den ? num : nullptr, divide && num != den ? len : 0, true, s);
    const fr_t* d_num = !divide ? nullptr : (num == den ? vden.d : vnum.d);
    dev_view* res = out == den ? &vden : (divide && out == num ? &vnum : nullptr);
    dev_view vout(res ? nullptr : out, res ? 0 : len, false, s);
    if (res == nullptr) res = &vout;
    poly_engine<fr_t>::inverse(res->d, d_num, vden.d, len, s);          // (synchronises the stream)
    vden.done(); vnum.done();
    res->flush();
}
}

SPPARK_FFI RustError sppark_field_inverse(size_t device_id, void* out, const void* inp, size_t len, void* stream)
{   return guarded([&] { field_inverse_any("sppark_field_inverse", device_id, out, nullptr, false, inp, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_divide(size_t device_id, void* out, const void* num, const void* den, size_t len, void* stream)
{   return guarded([&] { field_inverse_any("sppark_field_divide", device_id, out, num, true, den, len, (hipStream_t)stream); });   }
