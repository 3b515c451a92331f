// C entry points of the field-vector arithmetic over the library's field fr_t (include/sppark_amd_arith.h), and --
// in the libraries that have compute_ntt (SPPARK_VEC_WITH_NTT, set by api/ntt_api.hip) -- of the polynomial product and
// the vanishing quotient built from it and the transforms.
// Expects fr_t (and, with SPPARK_VEC_WITH_NTT, ntt_engine) in scope.
#pragma once
#include "call.hpp"
#include "../poly/vec_kernels.hpp"

namespace {
fr_t vec_zero() { fr_t z; memset(&z, 0, sizeof(z)); return z; }

template<int OP>
void vec_run(unsigned cus, fr_t* out, const fr_t* a, const fr_t* b, const fr_t* c, const fr_t& kval, const fr_t* kptr, size_t len, hipStream_t s)
{   vec_launch<fr_t, OP>(cus, out, a, b, c, kval, kptr, len, s);   }

void vec_dispatch(int op, unsigned cus, fr_t* out, const fr_t* a, const fr_t* b, const fr_t* c, const fr_t& kval, const fr_t* kptr, size_t len, hipStream_t s)
{
    switch (op) {
        case VEC_ADD:     vec_run<VEC_ADD>(cus, out, a, b, c, kval, kptr, len, s); break;
        case VEC_SUB:     vec_run<VEC_SUB>(cus, out, a, b, c, kval, kptr, len, s); break;
        case VEC_MUL:     vec_run<VEC_MUL>(cus, out, a, b, c, kval, kptr, len, s); break;
        case VEC_SCALE:   vec_run<VEC_SCALE>(cus, out, a, b, c, kval, kptr, len, s); break;
        case VEC_MUL_SUB: vec_run<VEC_MUL_SUB>(cus, out, a, b, c, kval, kptr, len, s); break;
        default:          vec_run<VEC_MUL_SUB_K>(cus, out, a, b, c, kval, kptr, len, s); break;
    }
}

// out = a (op) b ...; b, c, k: nullptr where the operation has no such operand.  Every argument is checked before a
// device is looked up.  All buffers on the device and a stream given: the call only enqueues.
void field_vec_any(const char* name, int op, size_t device_id, void* out, const void* a, const void* b, const void* c, const void* k,
                   size_t len, hipStream_t s)
{
    if (len == 0) return;
    const std::string who(name);
    const bool has_b = op != VEC_SCALE, has_c = op == VEC_MUL_SUB || op == VEC_MUL_SUB_K, has_k = op == VEC_SCALE || op == VEC_MUL_SUB_K;
    if (out == nullptr || a == nullptr || (has_b && b == nullptr) || (has_c && c == nullptr) || (has_k && k == nullptr))
        reject(who + ": NULL buffer with len > 0");
    const size_t bytes = elems_bytes(len, sizeof(fr_t), name);
    const std::string lap = who + ": buffers overlap partially (any two must be identical or disjoint)";
    const void* buf[4] = {out, a, has_b ? b : nullptr, has_c ? c : nullptr};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (buf[i] && buf[j]) same_or_disjoint(buf[i], buf[j], bytes, lap.c_str());
    if (has_k && ranges_meet(out, bytes, k, sizeof(fr_t))) reject(who + ": k may not overlap out");
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;

    fr_t kval = vec_zero();
    const fr_t* kptr = nullptr;
    if (has_k) { if (is_device_pointer(k)) kptr = (const fr_t*)k; else memcpy(&kval, k, sizeof(kval)); }

    call_scope sc(s);                                           // (identical buffers stay identical on the device)
    const fr_t* d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 1; i < 4; i++) if (buf[i]) d[i] = sc.in<fr_t>(buf[i], len);
    fr_t* d_out = sc.out<fr_t>(out, len);
    vec_dispatch(op, cus, d_out, d[1], d[2], d[3], kval, kptr, len, s);
    sc.finish();
}
}

SPPARK_FFI RustError sppark_field_add(size_t device_id, void* out, const void* a, const void* b, size_t len, void* stream)
{   return guarded([&] { field_vec_any("sppark_field_add", VEC_ADD, device_id, out, a, b, nullptr, nullptr, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_sub(size_t device_id, void* out, const void* a, const void* b, size_t len, void* stream)
{   return guarded([&] { field_vec_any("sppark_field_sub", VEC_SUB, device_id, out, a, b, nullptr, nullptr, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_mul(size_t device_id, void* out, const void* a, const void* b, size_t len, void* stream)
{   return guarded([&] { field_vec_any("sppark_field_mul", VEC_MUL, device_id, out, a, b, nullptr, nullptr, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_scale(size_t device_id, void* out, const void* a, const void* k, size_t len, void* stream)
{   return guarded([&] { field_vec_any("sppark_field_scale", VEC_SCALE, device_id, out, a, nullptr, nullptr, k, len, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_field_mul_sub(size_t device_id, void* out, const void* a, const void* b, const void* c, const void* k,
                                          size_t len, void* stream)
{
    return guarded([&] {
        field_vec_any("sppark_field_mul_sub", k ? VEC_MUL_SUB_K : VEC_MUL_SUB, device_id, out, a, b, c, k, len, (hipStream_t)stream);
    });
}

#ifdef SPPARK_VEC_WITH_NTT
namespace {
// (g^n - 1)^-1, n = 2^lg, g the generator of compute_ntt's Coset type: lg squarings and one inversion on the host
template<class F> F vanishing_inverse(unsigned lg)
{
    typedef host_field<F> H;
    auto gn = H::gen();
    for (unsigned i = 0; i < lg; i++) gn = H::mul(gn, gn);
    if constexpr (sizeof(F) <= 8) return H::wire(H::inv(gn ? gn - 1 : (decltype(gn))F::MOD - 1));     // (canonical integers)
    else { typename H::elem d{gn.v - H::one().v}; return H::wire(H::inv(d)); }
}

// out[0 .. la + lb - 1) = coefficients of (sum a_i x^i)(sum b_i x^i)
void poly_product_any(size_t device_id, void* out, const void* a, size_t la, const void* b, size_t lb, hipStream_t s)
{
    if (la == 0 || lb == 0) return;
    const std::string who("sppark_poly_product");
    if (out == nullptr || a == nullptr || b == nullptr) reject(who + ": NULL buffer with a length > 0");
    const size_t lo = checked_add(la, lb - 1, who.c_str(), ": la + lb - 1 overflows size_t");
    const size_t ob = elems_bytes(lo, sizeof(fr_t), who.c_str()), ab = elems_bytes(la, sizeof(fr_t), who.c_str()),
                 bb = elems_bytes(lb, sizeof(fr_t), who.c_str());
    unsigned lg = 0;
    while (lg < 63 && ((size_t)1 << lg) < lo) lg++;
    if (((size_t)1 << lg) < lo || lg > fr_t::TWO_ADICITY)
        reject(who + ": la + lb - 1 needs a transform above the field's 2-adicity of " + std::to_string(fr_t::TWO_ADICITY));
    if (ranges_meet(out, ob, a, ab) || ranges_meet(out, ob, b, bb)) reject(who + ": out must not overlap a or b");
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;
    const bool square = a == b && la == lb;
    const size_t n = (size_t)1 << lg;

    call_scope sc(s);
    const fr_t* d_a = sc.in<fr_t>(a, la);
    const fr_t* d_b = sc.in<fr_t>(b, lb);                       // (a square: the buffer of a)
    fr_t* d_out = sc.out<fr_t>(out, lo);
    const fr_t zero = vec_zero();
    if (lo <= 2) {                                              // no transform: one element times one or two
        if (la == 1) vec_launch<fr_t, VEC_SCALE>(cus, d_out, d_b, nullptr, nullptr, zero, d_a, lb, s);
        else         vec_launch<fr_t, VEC_SCALE>(cus, d_out, d_a, nullptr, nullptr, zero, d_b, la, s);
        sc.finish(true);
        return;
    }
    const size_t cols = square ? 1 : 2;
    fr_t* col = (fr_t*)sc.scratch(2 * n * sizeof(fr_t));
    const unsigned gx = (unsigned)std::min<size_t>((n + VEC_NT * 4 - 1) / (VEC_NT * 4), (size_t)std::max(cus, 1u) * VEC_WG_PER_CU);
    hipLaunchKernelGGL(k_vec_pad<fr_t>, dim3(gx, (unsigned)cols), dim3(VEC_NT), 0, s, col, n, d_a, la, d_b, lb);
    HIP_OK(hipGetLastError());
    auto& E = ntt_engine<fr_t>::instance();
    E.run(gpu, col, lg, NTT_NR, NTT_FORWARD, NTT_STANDARD, s, nullptr, cols, n);
    vec_launch<fr_t, VEC_MUL>(cus, col, col, square ? col : col + n, nullptr, zero, nullptr, n, s);
    E.run(gpu, col, lg, NTT_RN, NTT_INVERSE, NTT_STANDARD, s);
    HIP_OK(hipMemcpyAsync(d_out, col, ob, hipMemcpyDeviceToDevice, s));
    sc.finish(true);
}

// h = coefficients of (A B - C) / (x^n - 1) from the evaluations a, b, c over {w^i}
void vanishing_quotient_any(size_t device_id, void* h, const void* a, const void* b, const void* c, uint32_t lg, hipStream_t s)
{
    const std::string who("sppark_poly_vanishing_quotient");
    if (lg > fr_t::TWO_ADICITY)
        reject(who + ": lg_domain_size above the field's 2-adicity of " + std::to_string(fr_t::TWO_ADICITY));
    if (h == nullptr || a == nullptr || b == nullptr || c == nullptr) reject(who + ": NULL buffer");
    const size_t n = (size_t)1 << lg, bytes = elems_bytes(n, sizeof(fr_t), who.c_str());
    (void)elems_bytes(3 * n, sizeof(fr_t), who.c_str());
    const std::string lap = who + ": h overlaps an input partially (it must be identical to one or disjoint from all)";
    same_or_disjoint(h, a, bytes, lap.c_str()); same_or_disjoint(h, b, bytes, lap.c_str()); same_or_disjoint(h, c, bytes, lap.c_str());
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;

    // the three inputs go straight into the columns of the scratch and h comes straight out of it, from and to wherever they lie
    call_scope sc(s);
    fr_t* col = (fr_t*)sc.scratch(3 * bytes);
    const void* src[3] = {a, b, c};
    for (int j = 0; j < 3; j++) HIP_OK(hipMemcpyAsync(col + j * n, src[j], bytes, hipMemcpyDefault, s));
    auto& E = ntt_engine<fr_t>::instance();
    if (lg) {
        E.run(gpu, col, lg, NTT_NR, NTT_INVERSE, NTT_STANDARD, s, nullptr, 3, n);
        E.run(gpu, col, lg, NTT_RN, NTT_FORWARD, NTT_COSET, s, nullptr, 3, n);
    }
    vec_launch<fr_t, VEC_MUL_SUB_K>(cus, col, col, col + n, col + 2 * n, vanishing_inverse<fr_t>(lg), nullptr, n, s);
    if (lg) E.run(gpu, col, lg, NTT_NN, NTT_INVERSE, NTT_COSET, s);
    HIP_OK(hipMemcpyAsync(h, col, bytes, hipMemcpyDefault, s));
    sc.finish(true);
}
}

SPPARK_FFI RustError sppark_poly_product(size_t device_id, void* out, const void* a, size_t la, const void* b, size_t lb, void* stream)
{   return guarded([&] { poly_product_any(device_id, out, a, la, b, lb, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_poly_vanishing_quotient(size_t device_id, void* h, const void* a, const void* b, const void* c,
                                                    uint32_t lg_domain_size, void* stream)
{   return guarded([&] { vanishing_quotient_any(device_id, h, a, b, c, lg_domain_size, (hipStream_t)stream); });   }
#endif
