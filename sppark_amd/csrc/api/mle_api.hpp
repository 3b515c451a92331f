// C entry points of the multilinear tables and sumcheck rounds over the library's field fr_t (include/sppark_amd_mle.h).
// The launches are those of mle/mle_route.hpp: the drivers below run what the route says.
// Expects fr_t in scope.
#pragma once
#include "call.hpp"
#include "../mle/mle_kernels.hpp"

namespace {
// n = 2^lg_n elements in bytes; lg_n above MLE_MAX_LG is rejected
size_t mle_bytes(uint32_t lg_n, const std::string& who)
{
    if (lg_n > MLE_MAX_LG) reject(who + ": lg_n above " + std::to_string(MLE_MAX_LG));
    return elems_bytes((size_t)1 << lg_n, sizeof(fr_t), who.c_str());
}
int mle_order(int order, const std::string& who)
{
    if (order != MLE_LOW && order != MLE_HIGH) reject(who + ": unknown order");
    return order;
}
mle_route mle_route_of(const gpu_info& gpu, uint32_t lg_n, int op, unsigned rows, bool aligned16)
{
    mle_call c;
    c.elem_bytes = sizeof(fr_t); c.lg_n = lg_n; c.cus = (unsigned)gpu.prop.multiProcessorCount; c.op = op; c.rows = rows;
    c.aligned16 = aligned16;
    const mle_route r = make_mle_route(c);
    if (r.invalid) reject("sppark_mle: no route");
    return r;
}
bool mle_aligned16(std::initializer_list<const void*> ps)
{
    uintptr_t all = 0;
    for (const void* p : ps) all |= (uintptr_t)p;
    return (all & 15) == 0;
}

template<bool HIGH>
void mle_fold_launch(const mle_step& st, fr_t* out, const fr_t* in, const fr_t& rval, const fr_t* rptr, size_t half, hipStream_t s)
{
    const dim3 grid(st.grid), block(st.block);
    auto go = [&](auto VEC, auto KPTR) {
        hipLaunchKernelGGL((k_mle_fold<fr_t, HIGH, decltype(VEC)::value, decltype(KPTR)::value>), grid, block, 0, s, out, in, rval, rptr, half);
    };
    auto with_r = [&](auto VEC) { if (rptr != nullptr) go(VEC, std::true_type()); else go(VEC, std::false_type()); };
    if constexpr (sizeof(fr_t) < 16) { if (!st.vec) { with_r(std::false_type()); HIP_OK(hipGetLastError()); return; } }
    with_r(std::true_type());
    HIP_OK(hipGetLastError());
}

void mle_fold_any(size_t device_id, void* out, const void* in, uint32_t lg_n, const void* r, int order, hipStream_t s)
{
    const std::string who("sppark_mle_fold");
    const size_t bytes = mle_bytes(lg_n, who);
    if (lg_n == 0) reject(who + ": lg_n == 0 (nothing to bind)");
    mle_order(order, who);
    if (out == nullptr || in == nullptr || r == nullptr) reject(who + ": NULL buffer");
    const size_t half = (size_t)1 << (lg_n - 1);
    if (!(order == MLE_HIGH && out == in) && ranges_meet(out, bytes / 2, in, bytes))
        reject(who + (order == MLE_HIGH ? ": buffers overlap partially (HIGH: out must be identical to in or disjoint from it)"
                                         : ": buffers overlap (LOW: out must be disjoint from in)"));
    if (ranges_meet(out, bytes / 2, r, sizeof(fr_t))) reject(who + ": r may not overlap out");
    const gpu_info& gpu = select_gpu((int)device_id);

    fr_t rval;
    memset(&rval, 0, sizeof(rval));
    const fr_t* rptr = nullptr;
    if (is_device_pointer(r)) rptr = (const fr_t*)r; else memcpy(&rval, r, sizeof(rval));
    call_scope sc(s);
    const fr_t* d_in = sc.in<fr_t>(in, half * 2);
    fr_t* d_out = sc.out<fr_t>(out, half);                      // (half the size of in: on the host a buffer of its own even when out == in)
    const mle_route route = mle_route_of(gpu, lg_n, MLE_OP_FOLD, 0, mle_aligned16({d_out, d_in}));
    if (order == MLE_HIGH) mle_fold_launch<true>(route.steps[0], d_out, d_in, rval, rptr, half, s);
    else                   mle_fold_launch<false>(route.steps[0], d_out, d_in, rval, rptr, half, s);
    sc.finish();
}

void mle_bind_launch(const mle_step& st, fr_t* out, const fr_t* in, const fr_t* pt, hipStream_t s)
{
    const dim3 grid(st.grid), block(st.block);
    if constexpr (sizeof(fr_t) < 16) {
        if (!st.vec) { hipLaunchKernelGGL((k_mle_bind<fr_t, false>), grid, block, 0, s, out, in, pt, st.tile_lg, st.tiles); HIP_OK(hipGetLastError()); return; }
    }
    hipLaunchKernelGGL((k_mle_bind<fr_t, true>), grid, block, 0, s, out, in, pt, st.tile_lg, st.tiles);
    HIP_OK(hipGetLastError());
}

void mle_evaluate_any(size_t device_id, void* ret, const void* in, uint32_t lg_n, const void* point, hipStream_t s)
{
    const std::string who("sppark_mle_evaluate");
    const size_t bytes = mle_bytes(lg_n, who), n = (size_t)1 << lg_n;
    if (ret == nullptr || in == nullptr || (lg_n && point == nullptr)) reject(who + ": NULL buffer");
    if (ranges_meet(ret, sizeof(fr_t), in, bytes) || (lg_n && ranges_meet(ret, sizeof(fr_t), point, lg_n * sizeof(fr_t))))
        reject(who + ": ret may not overlap in or point");
    const gpu_info& gpu = select_gpu((int)device_id);

    if (lg_n == 0) {
        HIP_OK(hipMemcpyAsync(ret, in, sizeof(fr_t), hipMemcpyDefault, s));
        HIP_OK(hipStreamSynchronize(s));
        return;
    }
    call_scope sc(s);
    const fr_t* src = sc.in<fr_t>(in, n);
    const fr_t* d_pt = sc.in<fr_t>(point, lg_n);
    const mle_route route = mle_route_of(gpu, lg_n, MLE_OP_EVALUATE, 0, mle_aligned16({src}));
    fr_t* slot = (fr_t*)sc.scratch(route.scratch_elems * sizeof(fr_t));    // every pass writes behind the one before it; the last one one element
    const bool ret_dev = is_device_pointer(ret);
    for (unsigned i = 0; i < route.nsteps; i++) {
        const mle_step& st = route.steps[i];
        fr_t* dst = i + 1 == route.nsteps && ret_dev ? (fr_t*)ret : slot;
        mle_bind_launch(st, dst, src, d_pt + st.var_base, s);
        src = slot; slot += st.writes;
    }
    if (!ret_dev) sc.copy_out(ret, src, sizeof(fr_t));
    sc.finish(true);
}

void mle_eq_any(size_t device_id, void* out, const void* point, uint32_t lg_n, hipStream_t s)
{
    const std::string who("sppark_mle_eq");
    const size_t bytes = mle_bytes(lg_n, who), n = (size_t)1 << lg_n;
    if (out == nullptr || (lg_n && point == nullptr)) reject(who + ": NULL buffer");
    if (lg_n && ranges_meet(out, bytes, point, lg_n * sizeof(fr_t))) reject(who + ": out may not overlap point");
    const gpu_info& gpu = select_gpu((int)device_id);

    call_scope sc(s);
    const fr_t* d_pt = sc.in<fr_t>(point, lg_n);
    fr_t* d_out = sc.out<fr_t>(out, n);
    const mle_route route = mle_route_of(gpu, lg_n, MLE_OP_EQ, 0, mle_aligned16({d_out}));
    const mle_step& st = route.steps[0];
    const dim3 grid(st.grid), block(st.block);
    bool launched = false;
    if constexpr (sizeof(fr_t) < 16) {
        if (!st.vec) { hipLaunchKernelGGL((k_mle_eq<fr_t, false>), grid, block, 0, s, d_out, d_pt, lg_n, st.tile_lg, st.tiles); launched = true; }
    }
    if (!launched) hipLaunchKernelGGL((k_mle_eq<fr_t, true>), grid, block, 0, s, d_out, d_pt, lg_n, st.tile_lg, st.tiles);
    HIP_OK(hipGetLastError());
    sc.finish(true);
}

template<int NTAB, int FORM>
void sumcheck_round_launch(const mle_step& st, fr_t* slab, const mle_tables<fr_t>& tabs, size_t half, int order, hipStream_t s)
{
    const dim3 grid(st.grid), block(st.block);
    auto go = [&](auto HIGH, auto VEC) {
        hipLaunchKernelGGL((k_sumcheck_round<fr_t, NTAB, FORM, decltype(HIGH)::value, decltype(VEC)::value>), grid, block, 0, s, slab, tabs, half);
    };
    auto with_order = [&](auto VEC) { if (order == MLE_HIGH) go(std::true_type(), VEC); else go(std::false_type(), VEC); };
    if constexpr (sizeof(fr_t) < 16) { if (!st.vec) { with_order(std::false_type()); HIP_OK(hipGetLastError()); return; } }
    with_order(std::true_type());
    HIP_OK(hipGetLastError());
}

void sumcheck_round_any(size_t device_id, void* out, const void* const* tables, size_t ntables, int form, uint32_t lg_n, int order,
                        hipStream_t s)
{
    const std::string who("sppark_sumcheck_round");
    const size_t bytes = mle_bytes(lg_n, who), n = (size_t)1 << lg_n;
    if (lg_n == 0) reject(who + ": lg_n == 0 (no pairs)");
    mle_order(order, who);
    if (form != SUMCHECK_PRODUCT && form != SUMCHECK_EQ_MUL_SUB) reject(who + ": unknown form");
    if (form == SUMCHECK_PRODUCT ? (ntables < 1 || ntables > SUMCHECK_MAX_TABLES) : ntables != 4)
        reject(who + ": wrong ntables (PRODUCT: 1 .. 4, EQ_MUL_SUB: 4)");
    if (out == nullptr || tables == nullptr) reject(who + ": NULL buffer");
    for (size_t k = 0; k < ntables; k++) if (tables[k] == nullptr) reject(who + ": NULL table");
    const unsigned rows = form == SUMCHECK_PRODUCT ? (unsigned)ntables + 1 : 4;
    const std::string lap = who + ": tables overlap partially (any two must be identical or disjoint)";
    for (size_t i = 0; i < ntables; i++) {
        for (size_t j = i + 1; j < ntables; j++) same_or_disjoint(tables[i], tables[j], bytes, lap.c_str());
        if (ranges_meet(out, rows * sizeof(fr_t), tables[i], bytes)) reject(who + ": out may not overlap a table");
    }
    const gpu_info& gpu = select_gpu((int)device_id);

    call_scope sc(s);                                           // (identical tables stay identical on the device)
    mle_tables<fr_t> tabs;
    bool aligned = true;
    for (size_t k = 0; k < SUMCHECK_MAX_TABLES; k++) {
        tabs.p[k] = k < ntables ? sc.in<fr_t>(tables[k], n) : tabs.p[0];
        aligned = aligned && mle_aligned16({tabs.p[k]});
    }
    const mle_route route = mle_route_of(gpu, lg_n, MLE_OP_ROUND, rows, aligned);
    fr_t* slab = (fr_t*)sc.scratch(route.scratch_elems * sizeof(fr_t));
    fr_t* sums = slab + route.steps[0].writes;
    const bool out_dev = is_device_pointer(out);
    const mle_step& st = route.steps[0];
    const size_t half = n / 2;
    if (form == SUMCHECK_EQ_MUL_SUB) sumcheck_round_launch<4, SUMCHECK_EQ_MUL_SUB>(st, slab, tabs, half, order, s);
    else if (ntables == 1) sumcheck_round_launch<1, SUMCHECK_PRODUCT>(st, slab, tabs, half, order, s);
    else if (ntables == 2) sumcheck_round_launch<2, SUMCHECK_PRODUCT>(st, slab, tabs, half, order, s);
    else if (ntables == 3) sumcheck_round_launch<3, SUMCHECK_PRODUCT>(st, slab, tabs, half, order, s);
    else                   sumcheck_round_launch<4, SUMCHECK_PRODUCT>(st, slab, tabs, half, order, s);
    const mle_step& sum = route.steps[1];
    hipLaunchKernelGGL((k_sumcheck_sum<fr_t>), dim3(sum.grid), dim3(sum.block), 0, s, out_dev ? (fr_t*)out : sums, slab, sum.tiles, rows);
    HIP_OK(hipGetLastError());
    if (!out_dev) sc.copy_out(out, sums, rows * sizeof(fr_t));
    sc.finish(true);
}
}

SPPARK_FFI RustError sppark_mle_fold(size_t device_id, void* out, const void* in, uint32_t lg_n, const void* r, int order, void* stream)
{   return guarded([&] { mle_fold_any(device_id, out, in, lg_n, r, order, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_mle_evaluate(size_t device_id, void* ret, const void* in, uint32_t lg_n, const void* point, void* stream)
{   return guarded([&] { mle_evaluate_any(device_id, ret, in, lg_n, point, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_mle_eq(size_t device_id, void* out, const void* point, uint32_t lg_n, void* stream)
{   return guarded([&] { mle_eq_any(device_id, out, point, lg_n, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_sumcheck_round(size_t device_id, void* out, const void* const* tables, size_t ntables, int form, uint32_t lg_n,
                                           int order, void* stream)
{   return guarded([&] { sumcheck_round_any(device_id, out, tables, ntables, form, lg_n, order, (hipStream_t)stream); });   }
