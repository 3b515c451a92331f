// C entry points of the polynomial primitives over the library's field fr_t (included by
// api/ntt_api.hip for the NTT-capable libraries and by api/poly_only_api.hip for fields that have
// no NTT parameters in the reference: Mersenne31, the BabyBear quartic extension).
// Expects fr_t in scope.  Host buffers are staged by a call_scope (api/call.hpp); the poly_engine functions
// synchronise the stream themselves and take their own scratch.
#pragma once
#include "call.hpp"
#include "../poly/poly_driver.hpp"

// ---- polynomial primitives over this library's field (C++ templates only in the reference:
// polynomial/prefix_op.cuh, evaluate.cuh, div_by_x_minus_z.cuh) ---------------------------------
SPPARK_FFI RustError sppark_prefix_op(size_t device_id, void* out, const void* inp, size_t len, int op, void* stream)
{
    return guarded([&] {
        (void)select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        if (len == 0) return;
        call_scope sc(s);
        const fr_t* d_in = sc.in<fr_t>(inp, len);
        fr_t* d_out = sc.out<fr_t>(out, len);                       // (out == inp: the same buffer, in place)
        poly_engine<fr_t>::prefix_op(d_out, d_in, len, op, s);
        sc.finish();
    });
}

SPPARK_FFI RustError sppark_poly_evaluate(size_t device_id, void* ret, const void* x, size_t n,
                                          const void* coeffs, size_t len, void* stream)
{
    return guarded([&] {
        (void)select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        if (n == 0) return;
        call_scope sc(s);
        const fr_t* d_x = sc.in<fr_t>(x, n);
        const fr_t* d_c = sc.in<fr_t>(coeffs, len);
        fr_t* d_ret = sc.out<fr_t>(ret, n);
        poly_engine<fr_t>::evaluate(d_ret, d_x, n, d_c, len, s);
        sc.finish();
    });
}

SPPARK_FFI RustError sppark_div_by_x_minus_z(size_t device_id, void* inout, size_t len, const void* z, int rotate, void* stream)
{
    return guarded([&] {
        (void)select_gpu((int)device_id);
        hipStream_t s = (hipStream_t)stream;
        if (len == 0) return;
        if (z == nullptr) HIP_OK(hipErrorInvalidValue);
        fr_t zv;
        if (is_device_pointer(z)) HIP_OK(hipMemcpy(&zv, z, sizeof(zv), hipMemcpyDeviceToHost));
        else memcpy(&zv, z, sizeof(zv));
        call_scope sc(s);
        fr_t* d = sc.inout<fr_t>(inout, len);
        poly_engine<fr_t>::div_by_x_minus_z(d, len, zv, rotate != 0, s);
        sc.finish();
    });
}
