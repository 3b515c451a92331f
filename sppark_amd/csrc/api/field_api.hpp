// C entry points of the field-vector inverse and quotient over the library's field fr_t
// (include/sppark_amd_field.h; the reference's ff/batch_inversion.hpp is a host-side C++ template).
// Expects fr_t in scope.
#pragma once
#include "call.hpp"
#include "../poly/poly_driver.hpp"

namespace {
// out[i] = num[i] / den[i] (num == nullptr: 1 / den[i]); every argument is checked before a device is looked up
void field_inverse_any(const char* name, size_t device_id, void* out, const void* num, bool divide, const void* den, size_t len, hipStream_t s)
{
    if (len == 0) return;
    const std::string who(name);
    if (out == nullptr || den == nullptr || (divide && num == nullptr)) reject(who + ": NULL buffer with len > 0");
    const size_t bytes = elems_bytes(len, sizeof(fr_t), name);
    const std::string lap = who + ": buffers overlap partially (any two must be identical or disjoint)";
    same_or_disjoint(out, den, bytes, lap.c_str());
    if (divide) { same_or_disjoint(out, num, bytes, lap.c_str()); same_or_disjoint(num, den, bytes, lap.c_str()); }
    (void)select_gpu((int)device_id);

    call_scope sc(s);
    const fr_t* d_den = sc.in<fr_t>(den, len);
    const fr_t* d_num = divide ? sc.in<fr_t>(num, len) : nullptr;
    fr_t* d_out = sc.out<fr_t>(out, len);
    poly_engine<fr_t>::inverse(d_out, d_num, d_den, len, s);            // (synchronises the stream)
    sc.finish();
}
}

SPPARK_FFI RustError sppark_field_inverse(size_t device_id, void* out, const void* inp, size_t len, void* stream)
{   return guarded([&] { field_inverse_any("sppark_field_inverse", device_id, out, nullptr, false, inp, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_divide(size_t device_id, void* out, const void* num, const void* den, size_t len, void* stream)
{   return guarded([&] { field_inverse_any("sppark_field_divide", device_id, out, num, true, den, len, (hipStream_t)stream); });   }
