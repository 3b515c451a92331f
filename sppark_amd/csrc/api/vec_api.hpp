// C entry points of the field-vector arithmetic over the library's field fr_t (include/sppark_amd_arith.h), and --
// in the libraries that have compute_ntt (SPPARK_VEC_WITH_NTT, set by api/ntt_api.hip) -- of the polynomial product and
// the vanishing quotient built from it and the transforms.  Included behind api/field_api.hpp, whose argument checks
// (field_reject, field_check_pair) and whose dev_view staging it shares.
// Expects: fr_t, guarded(), SPPARK_FFI, select_gpu, is_device_pointer in scope.
#pragma once
#include "field_api.hpp"
#include "../poly/vec_kernels.hpp"
#include <memory>

namespace {
// [p, p + pb) and [q, q + qb) share a byte
bool vec_ranges_meet(const void* p, size_t pb, const void* q, size_t qb)
{
    const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
    return x < y ? y - x < pb : x - y < qb;
}
size_t vec_bytes(size_t len, const std::string& who)
{
    size_t bytes = 0;
    if (__builtin_mul_overflow(len, sizeof(fr_t), &bytes)) field_reject((who + ": len * sizeof(element) overflows size_t").c_str());
    return bytes;
}
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
        field_reject((who + ": NULL buffer with len > 0").c_str());
    const size_t bytes = vec_bytes(len, who);
    const std::string lap = who + ": buffers overlap partially (any two must be identical or disjoint)";
    const void* buf[4] = {out, a, has_b ? b : nullptr, has_c ? c : nullptr};
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (buf[i] && buf[j]) field_check_pair(buf[i], buf[j], bytes, lap.c_str());
    if (has_k && vec_ranges_meet(out, bytes, k, sizeof(fr_t))) field_reject((who + ": k may not overlap out").c_str());
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;

    fr_t kval = vec_zero();
    const fr_t* kptr = nullptr;
    if (has_k) { if (is_device_pointer(k)) kptr = (const fr_t*)k; else memcpy(&kval, k, sizeof(kval)); }

    bool all_dev = true;
    for (int i = 0; i < 4; i++) if (buf[i] && !is_device_pointer(buf[i])) all_dev = false;
    if (all_dev) {
        vec_dispatch(op, cus, (fr_t*)out, (const fr_t*)a, (const fr_t*)b, (const fr_t*)c, kval, kptr, len, s);
        if (s == nullptr) HIP_OK(hipStreamSynchronize(s));
        return;
    }
    // a host buffer among them: one device view per DISTINCT buffer (identical pointers stay identical on the device)
    std::unique_ptr<dev_view> view[4];
    fr_t* d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 1; i < 4; i++) {
        if (!buf[i]) continue;
        int same = 0;
        for (int j = 1; j < i; j++) if (buf[j] == buf[i]) same = j;
        if (same) { d[i] = d[same]; continue; }
        view[i].reset(new dev_view(buf[i], len, true, s));
        d[i] = view[i]->d;
    }
    int alias = 0;                                              // the first input that out is (its view was made above)
    for (int i = 3; i >= 1; i--) if (buf[i] == out) alias = i;
    if (!alias) view[0].reset(new dev_view(out, len, false, s));
    dev_view* res = view[alias].get();
    d[0] = res->d;
    vec_dispatch(op, cus, d[0], d[1], d[2], d[3], kval, kptr, len, s);
    if (res->owned) res->flush();                               // (synchronises the stream)
    else HIP_OK(hipStreamSynchronize(s));
    for (int i = 0; i < 4; i++) if (view[i]) view[i]->done();
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
    if (out == nullptr || a == nullptr || b == nullptr) field_reject((who + ": NULL buffer with a length > 0").c_str());
    size_t lo = 0;
    if (__builtin_add_overflow(la, lb - 1, &lo)) field_reject((who + ": la + lb - 1 overflows size_t").c_str());
    const size_t ob = vec_bytes(lo, who), ab = vec_bytes(la, who), bb = vec_bytes(lb, who);
    unsigned lg = 0;
    while (lg < 63 && ((size_t)1 << lg) < lo) lg++;
    if (((size_t)1 << lg) < lo || lg > fr_t::TWO_ADICITY)
        field_reject((who + ": la + lb - 1 needs a transform above the field's 2-adicity of " + std::to_string(fr_t::TWO_ADICITY)).c_str());
    if (vec_ranges_meet(out, ob, a, ab) || vec_ranges_meet(out, ob, b, bb))
        field_reject((who + ": out must not overlap a or b").c_str());
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;
    const bool square = a == b && la == lb;
    const size_t n = (size_t)1 << lg;

    dev_view va(a, la, true, s), vb(square ? nullptr : b, square ? 0 : lb, true, s), vo(out, lo, false, s);
    const fr_t* d_a = va.d;
    const fr_t* d_b = square ? va.d : vb.d;
    const fr_t zero = vec_zero();
    if (lo <= 2) {                                              // no transform: one element times one or two
        if (la == 1) vec_launch<fr_t, VEC_SCALE>(cus, vo.d, d_b, nullptr, nullptr, zero, d_a, lb, s);
        else         vec_launch<fr_t, VEC_SCALE>(cus, vo.d, d_a, nullptr, nullptr, zero, d_b, la, s);
        if (vo.owned) vo.flush(); else HIP_OK(hipStreamSynchronize(s));
        va.done(); vb.done();
        return;
    }
    const size_t cols = square ? 1 : 2;
    pooled_scratch buf(2 * n * sizeof(fr_t));
    fr_t* col = (fr_t*)buf.p;
    const unsigned gx = (unsigned)std::min<size_t>((n + VEC_NT * 4 - 1) / (VEC_NT * 4), (size_t)std::max(cus, 1u) * VEC_WG_PER_CU);
    hipLaunchKernelGGL(k_vec_pad<fr_t>, dim3(gx, (unsigned)cols), dim3(VEC_NT), 0, s, col, n, d_a, la, d_b, lb);
    HIP_OK(hipGetLastError());
    auto& E = ntt_engine<fr_t>::instance();
    E.run(gpu, col, lg, NTT_NR, NTT_FORWARD, NTT_STANDARD, s, nullptr, cols, n);
    vec_launch<fr_t, VEC_MUL>(cus, col, col, square ? col : col + n, nullptr, zero, nullptr, n, s);
    E.run(gpu, col, lg, NTT_RN, NTT_INVERSE, NTT_STANDARD, s);
    HIP_OK(hipMemcpyAsync(vo.d, col, ob, hipMemcpyDeviceToDevice, s));
    if (vo.owned) vo.flush(); else HIP_OK(hipStreamSynchronize(s));
    va.done(); vb.done();
    buf.done();
}

// h = coefficients of (A B - C) / (x^n - 1) from the evaluations a, b, c over {w^i}
void vanishing_quotient_any(size_t device_id, void* h, const void* a, const void* b, const void* c, uint32_t lg, hipStream_t s)
{
    const std::string who("sppark_poly_vanishing_quotient");
    if (lg > fr_t::TWO_ADICITY)
        field_reject((who + ": lg_domain_size above the field's 2-adicity of " + std::to_string(fr_t::TWO_ADICITY)).c_str());
    if (h == nullptr || a == nullptr || b == nullptr || c == nullptr) field_reject((who + ": NULL buffer").c_str());
    const size_t n = (size_t)1 << lg, bytes = vec_bytes(n, who);
    (void)vec_bytes(3 * n, who);
    const std::string lap = who + ": h overlaps an input partially (it must be identical to one or disjoint from all)";
    field_check_pair(h, a, bytes, lap.c_str()); field_check_pair(h, b, bytes, lap.c_str()); field_check_pair(h, c, bytes, lap.c_str());
    const gpu_info& gpu = select_gpu((int)device_id);
    const unsigned cus = (unsigned)gpu.prop.multiProcessorCount;

    pooled_scratch buf(3 * bytes);
    fr_t* col = (fr_t*)buf.p;
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
    HIP_OK(hipStreamSynchronize(s));
    buf.done();
}
}

SPPARK_FFI RustError sppark_poly_product(size_t device_id, void* out, const void* a, size_t la, const void* b, size_t lb, void* stream)
{   return guarded([&] { poly_product_any(device_id, out, a, la, b, lb, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_poly_vanishing_quotient(size_t device_id, void* h, const void* a, const void* b, const void* c,
                                                    uint32_t lg_domain_size, void* stream)
{   return guarded([&] { vanishing_quotient_any(device_id, h, a, b, c, lg_domain_size, (hipStream_t)stream); });   }
#endif
