// C entry points of the FRI calls over the library's field fr_t (include/sppark_amd_fri.h): fold, reduce, domain.
// The launch is that of fri/fri_route.hpp: the drivers below run what the route says, with the constants of the domain
// computed here on the host (host_field of ntt/ntt_driver.hpp).
// Expects fr_t in scope.  Libraries without a 2-adic domain (-DFEATURE_MERSENNE31) get sppark_fri_reduce only.
#pragma once
#include "call.hpp"
#include "../fri/fri_kernels.hpp"
#if !defined(FEATURE_MERSENNE31)
# include "../ntt/ntt_driver.hpp"       // host_field
# define SPPARK_FRI_HAS_DOMAIN 1
#endif

namespace {
constexpr const char* FRI_OVERFLOW = ": a size overflows size_t";

bool fri_aligned16(std::initializer_list<const void*> ps)
{
    uintptr_t all = 0;
    for (const void* p : ps) all |= (uintptr_t)p;
    return (all & 15) == 0;
}

#ifdef SPPARK_FRI_HAS_DOMAIN
typedef fri_base<fr_t>::type fri_b;                             // the field of the domain's points

// host arithmetic on the domain's field: canonical integers (single-word fields) or Montgomery elements (256-bit fields)
template<class B> struct fri_host_t {
    typedef host_field<B> H;
    typedef decltype(H::top_root()) E;
    static E one() { if constexpr (sizeof(B) <= 8) return (E)1; else return H::one(); }
    static E two() { if constexpr (sizeof(B) <= 8) return (E)2; else return H::small(2); }
    static bool is_one(const E& e) { if constexpr (sizeof(B) <= 8) return e == (E)1; else return e.v == H::one().v; }
    static const E& half() { static const E h = H::inv(two()); return h; }         // (an inversion: once per process)
    static E root(unsigned lg)
    {
        static const E top = H::top_root();                                         // (a 256-bit field's takes hundreds of products)
        E w = top;
        for (unsigned k = B::TWO_ADICITY; k > lg; k--) w = H::mul(w, w);
        return w;
    }
    // one element in wire form on the host; false: zero or not canonical
    static bool from_wire(const void* p, E& e)
    {
        if constexpr (sizeof(B) == 8) { u64 v; memcpy(&v, p, 8); e = v; return v != 0 && v < B::MOD; }
        else if constexpr (sizeof(B) == 4) {                        // a Montgomery word: out of Montgomery form
            u32 v; memcpy(&v, p, 4);
            static const E rinv = H::inv(((u64)1 << 32) % B::MOD);  // (an inversion: once per process)
            e = H::mul(v, rinv);
            return v != 0 && v < B::MOD;
        } else { memcpy(e.v.v, p, sizeof(e.v.v)); return !e.v.is_zero(); }
    }
    // 1 / shift.  A prover folds layer after layer with few distinct shifts: the last one's inverse is kept per thread, so
    // that a fold with the shift of the call before costs no inversion on the host.
    static E shift_inverse(const E& shift)
    {
        if (is_one(shift)) return shift;
        static thread_local bool have = false;
        static thread_local E last, last_inv;
        if (!have || memcmp(&last, &shift, sizeof(E)) != 0) { last_inv = H::inv(shift); last = shift; have = true; }
        return last_inv;
    }
};
typedef fri_host_t<fri_b> fri_host;

unsigned fri_lg_of(uint32_t lg_n, const std::string& who)
{
    if (lg_n > FRI_MAX_LG) reject(who + ": lg_n above " + std::to_string(FRI_MAX_LG));
    if (lg_n > fri_b::TWO_ADICITY) reject(who + ": lg_n above the field's 2-adicity of " + std::to_string(fri_b::TWO_ADICITY));
    return lg_n;
}
bool fri_bitrev_of(int order, const std::string& who)
{
    if (order != FRI_NATURAL && order != FRI_BITREV) reject(who + ": unknown order");
    return order == FRI_BITREV;
}
fri_host::E fri_shift_of(const void* shift, const std::string& who)
{
    fri_host::E sh = fri_host::one();
    if (shift != nullptr && !fri_host::from_wire(shift, sh)) reject(who + ": shift is zero or not canonical");
    return sh;
}
fri_route fri_route_of(const gpu_info& gpu, int op, uint32_t lg_n, unsigned lg_arity, int order, bool aligned16, fri_geom& g)
{
    fri_call c;
    c.elem_bytes = sizeof(fr_t); c.lg_n = lg_n; c.cus = (unsigned)gpu.prop.multiProcessorCount; c.op = op; c.lg_arity = lg_arity;
    c.order = order; c.aligned16 = aligned16;
    const fri_route r = make_fri_route(c);
    if (r.invalid) reject("sppark_fri: no route");
    g = fri_geom{lg_n - (op == FRI_OP_FOLD ? lg_arity : 0), r.out_lg, r.tile_bits, r.grid_lg};
    return r;
}

// the constants of one launch: inverse (fold) or forward (domain) powers of the root of order 2^lg_n
template<unsigned CN>
fri_consts<fri_b, CN> fri_consts_of(bool inverse, bool bitrev, const fri_geom& g, unsigned lg_n, unsigned lg_arity, fri_host::E shift,
                                    unsigned pack)
{
    typedef fri_host HF;
    typedef HF::H H;
    // sq[j] = r^(2^j) for r = w or, without an inversion, w^-1 = w^(n - 1); every power below is a product of some of them
    HF::E sq[FRI_MAX_LG + 1];
    sq[0] = HF::root(lg_n);
    if (inverse) {
        HF::E p = sq[0], acc = HF::one();
        for (unsigned j = 0; j < lg_n; j++) { acc = H::mul(acc, p); p = H::mul(p, p); }
        sq[0] = acc;
        shift = HF::shift_inverse(shift);
    }
    for (unsigned j = 1; j <= FRI_MAX_LG; j++) sq[j] = H::mul(sq[j - 1], sq[j - 1]);
    auto power = [&](u64 e) { HF::E r = HF::one(); for (unsigned j = 0; e; j++, e >>= 1) if (e & 1) r = H::mul(r, sq[j]); return r; };

    fri_consts<fri_b, CN> k;
    k.base = H::wire(shift);
    k.step = H::wire(power(fri_step_exp(bitrev, g)));
    HF::E scale = HF::one();
    for (unsigned l = 0; l < lg_arity; l++) scale = H::mul(scale, HF::half());
    k.scale = H::wire(scale);
    for (unsigned t = 0; t < 4; t++)                                // zeta = r^(2^lg_m), of order 2^lg_arity
        k.z[t] = H::wire(lg_arity && t < (1u << (lg_arity - 1)) ? power(fri_bitrev(t, lg_arity - 1) << g.lg_m) : HF::one());
    for (unsigned c = 0; c < CN; c++) k.c[c] = H::wire(power(fri_const_exp(bitrev, g, c / pack, c % pack, pack)));
    // the digit tables: entry i is the product of the entries of i's set bits, each a single sq[j]
    auto table = [&](fri_b* tab, unsigned d, bool of_group) {
        HF::E v[16];
        v[0] = HF::one();
        for (unsigned j = 0; j < 4; j++) {
            const unsigned x = 1u << (4 * d + j);
            const HF::E gen = of_group ? (x >> g.grid_lg ? HF::one() : power(fri_lane_exp(bitrev, g, x, 0, pack)))
                                       : power(fri_lane_exp(bitrev, g, 0, x, pack));
            for (unsigned i = 0; i < (1u << j); i++) v[i | (1u << j)] = H::mul(v[i], gen);
        }
        for (unsigned i = 0; i < 16; i++) tab[i] = H::wire(v[i]);
    };
    for (unsigned d = 0; d < 2; d++) table(k.tt[d], d, false);
    for (unsigned d = 0; d < 3; d++) table(k.tb[d], d, true);
    return k;
}

template<unsigned LGA, bool BITREV, bool VEC>
void fri_fold_launch(const fri_route& r, const fri_geom& g, fr_t* out, const fr_t* in, const fr_t& bval, const fr_t* bptr, unsigned lg_n,
                     fri_host::E shift, hipStream_t s)
{
    typedef fri_fold_shape<fr_t, LGA, VEC> S;
    const auto k = fri_consts_of<S::CN>(true, BITREV, g, lg_n, LGA, shift, S::N);
    hipLaunchKernelGGL((k_fri_fold<fr_t, LGA, BITREV, VEC>), dim3(r.grid), dim3(r.block), 0, s, out, in, bval, bptr, k, g);
    HIP_OK(hipGetLastError());
}
template<unsigned LGA>
void fri_fold_pick(const fri_route& r, const fri_geom& g, bool bitrev, fr_t* out, const fr_t* in, const fr_t& bval, const fr_t* bptr,
                   unsigned lg_n, fri_host::E shift, hipStream_t s)
{
    if constexpr (sizeof(fr_t) < 16) {
        if (!r.vec) {
            if (bitrev) fri_fold_launch<LGA, true, false>(r, g, out, in, bval, bptr, lg_n, shift, s);
            else        fri_fold_launch<LGA, false, false>(r, g, out, in, bval, bptr, lg_n, shift, s);
            return;
        }
    }
    if (bitrev) fri_fold_launch<LGA, true, true>(r, g, out, in, bval, bptr, lg_n, shift, s);
    else        fri_fold_launch<LGA, false, true>(r, g, out, in, bval, bptr, lg_n, shift, s);
}

void fri_fold_any(size_t device_id, void* out, const void* in, uint32_t lg_n, uint32_t lg_arity, const void* beta, const void* shift,
                  int order, hipStream_t s)
{
    const std::string who("sppark_fri_fold");
    fri_lg_of(lg_n, who);
    if (lg_arity < 1 || lg_arity > FRI_MAX_LG_ARITY) reject(who + ": lg_arity outside 1 .. " + std::to_string(FRI_MAX_LG_ARITY));
    if (lg_n < lg_arity) reject(who + ": lg_n below lg_arity");
    const bool bitrev = fri_bitrev_of(order, who);
    if (out == nullptr || in == nullptr || beta == nullptr) reject(who + ": NULL buffer");
    const size_t n = (size_t)1 << lg_n, m = n >> lg_arity;
    const size_t bytes = elems_bytes(n, sizeof(fr_t), who.c_str()), out_bytes = bytes >> lg_arity;
    if (!(!bitrev && out == in) && ranges_meet(out, out_bytes, in, bytes))
        reject(who + (bitrev ? ": buffers overlap (BITREV: out must be disjoint from in)"
                             : ": buffers overlap partially (NATURAL: out must be identical to in or disjoint from it)"));
    if (ranges_meet(out, out_bytes, beta, sizeof(fr_t))) reject(who + ": beta may not overlap out");
    const fri_host::E sh = fri_shift_of(shift, who);
    const gpu_info& gpu = select_gpu((int)device_id);

    fr_t bval;
    memset(&bval, 0, sizeof(bval));
    const fr_t* bptr = nullptr;
    if (is_device_pointer(beta)) bptr = (const fr_t*)beta; else memcpy(&bval, beta, sizeof(bval));
    call_scope sc(s);
    const fr_t* d_in = sc.in<fr_t>(in, n);
    fr_t* d_out = sc.out<fr_t>(out, m);                         // (on the host a buffer of its own even when out == in)
    fri_geom g;
    const fri_route r = fri_route_of(gpu, FRI_OP_FOLD, lg_n, lg_arity, order, fri_aligned16({d_out, d_in}), g);
    if (lg_arity == 1)      fri_fold_pick<1>(r, g, bitrev, d_out, d_in, bval, bptr, lg_n, sh, s);
    else if (lg_arity == 2) fri_fold_pick<2>(r, g, bitrev, d_out, d_in, bval, bptr, lg_n, sh, s);
    else                    fri_fold_pick<3>(r, g, bitrev, d_out, d_in, bval, bptr, lg_n, sh, s);
    sc.finish();
}

template<bool BITREV, bool VEC>
void fri_domain_launch(const fri_route& r, const fri_geom& g, fr_t* out, const fr_t& zval, const fr_t* zptr, unsigned lg_n, fri_host::E shift,
                       hipStream_t s)
{
    typedef fri_domain_shape<fr_t, VEC> S;
    const auto k = fri_consts_of<S::CN>(false, BITREV, g, lg_n, 0, shift, S::N);
    hipLaunchKernelGGL((k_fri_domain<fr_t, BITREV, VEC>), dim3(r.grid), dim3(r.block), 0, s, out, zval, zptr, k, g);
    HIP_OK(hipGetLastError());
}

void fri_domain_any(size_t device_id, void* out, uint32_t lg_n, const void* shift, int order, const void* z, hipStream_t s)
{
    const std::string who("sppark_fri_domain");
    fri_lg_of(lg_n, who);
    const bool bitrev = fri_bitrev_of(order, who);
    if (out == nullptr) reject(who + ": NULL out");
    const size_t n = (size_t)1 << lg_n, bytes = elems_bytes(n, sizeof(fr_t), who.c_str());
    if (z != nullptr && ranges_meet(out, bytes, z, sizeof(fr_t))) reject(who + ": z may not overlap out");
    const fri_host::E sh = fri_shift_of(shift, who);
    const gpu_info& gpu = select_gpu((int)device_id);

    fr_t zval;
    memset(&zval, 0, sizeof(zval));
    const fr_t* zptr = nullptr;
    if (z != nullptr) { if (is_device_pointer(z)) zptr = (const fr_t*)z; else memcpy(&zval, z, sizeof(zval)); }
    call_scope sc(s);
    fr_t* d_out = sc.out<fr_t>(out, n);
    fri_geom g;
    const fri_route r = fri_route_of(gpu, FRI_OP_DOMAIN, lg_n, 0, order, fri_aligned16({d_out}), g);
    bool launched = false;
    if constexpr (sizeof(fr_t) < 16) {
        if (!r.vec) {
            if (bitrev) fri_domain_launch<true, false>(r, g, d_out, zval, zptr, lg_n, sh, s);
            else        fri_domain_launch<false, false>(r, g, d_out, zval, zptr, lg_n, sh, s);
            launched = true;
        }
    }
    if (!launched) {
        if (bitrev) fri_domain_launch<true, true>(r, g, d_out, zval, zptr, lg_n, sh, s);
        else        fri_domain_launch<false, true>(r, g, d_out, zval, zptr, lg_n, sh, s);
    }
    sc.finish();
}
#endif  // SPPARK_FRI_HAS_DOMAIN

// ---- reduce ----
template<class E, bool COLS>
void fri_reduce_launch(const fri_route& r, fr_t* out, const E* in, const fr_t* w, size_t n, size_t width, size_t cs, size_t ls,
                       const fr_t& subval, const fr_t* subptr, int accumulate, hipStream_t s)
{
    const dim3 grid(r.grid), block(r.block);
    bool launched = false;
    if constexpr (sizeof(E) < 16) {
        if (!r.vec) {
            hipLaunchKernelGGL((k_fri_reduce<fr_t, E, COLS, false>), grid, block, 0, s, out, in, w, n, width, cs, ls, subval, subptr, accumulate);
            launched = true;
        }
    }
    if (!launched) hipLaunchKernelGGL((k_fri_reduce<fr_t, E, COLS, true>), grid, block, 0, s, out, in, w, n, width, cs, ls, subval, subptr, accumulate);
    HIP_OK(hipGetLastError());
}

template<class E>
void fri_reduce_run(const gpu_info& gpu, call_scope& sc, void* out, const void* in, uint32_t lg_n, size_t width, size_t cs, size_t ls,
                    bool cols, const void* weights, const void* sub, int accumulate, hipStream_t s)
{
    const size_t n = (size_t)1 << lg_n;
    fr_t subval;
    memset(&subval, 0, sizeof(subval));
    const fr_t* subptr = nullptr;
    if (sub != nullptr) { if (is_device_pointer(sub)) subptr = (const fr_t*)sub; else memcpy(&subval, sub, sizeof(subval)); }
    // a host matrix arrives packed: only its elements are read, never the gaps of a stride
    const E* d_in = sc.in_lines<E>(in, cols ? n : width, cols ? width : n, cols ? cs : ls);
    if ((const void*)d_in != in) { if (cols) cs = n; else ls = width; }
    const fr_t* d_w = sc.in<fr_t>(weights, width);
    fr_t* d_out = accumulate ? sc.inout<fr_t>(out, n) : sc.out<fr_t>(out, n);
    fri_call c;
    c.elem_bytes = sizeof(E); c.lg_n = lg_n; c.cus = (unsigned)gpu.prop.multiProcessorCount; c.op = FRI_OP_REDUCE;
    c.layout = cols ? FRI_COLUMNS : FRI_ROWS; c.width = width;
    c.aligned16 = fri_aligned16({d_in}) && (((cols ? cs : ls) * sizeof(E)) & 15) == 0;
    const fri_route r = make_fri_route(c);
    if (r.invalid) reject("sppark_fri_reduce: no route");
    if (cols) fri_reduce_launch<E, true>(r, d_out, d_in, d_w, n, width, cs, ls, subval, subptr, accumulate, s);
    else      fri_reduce_launch<E, false>(r, d_out, d_in, d_w, n, width, cs, ls, subval, subptr, accumulate, s);
}

void fri_reduce_any(size_t device_id, void* out, const void* in, int in_base, uint32_t lg_n, size_t width, size_t col_stride,
                    size_t leaf_stride, const void* weights, const void* sub, int accumulate, hipStream_t s)
{
    const std::string who("sppark_fri_reduce");
    const char* w = who.c_str();
    if (out == nullptr || in == nullptr || weights == nullptr) reject(who + ": NULL buffer");
    if (lg_n > FRI_MAX_LG) reject(who + ": lg_n above " + std::to_string(FRI_MAX_LG));
    if (width == 0) reject(who + ": width == 0");
    if (in_base != 0 && in_base != 1) reject(who + ": in_base is 0 or 1");
#if defined(FEATURE_BABY_BEAR_X4)
    const size_t es = in_base ? sizeof(bb31_dev) : sizeof(fr_t);
#else
    if (in_base) reject(who + ": in_base == 1 needs a library over an extension field (libsppark_bb31x4)");
    const size_t es = sizeof(fr_t);
#endif
    const size_t n = (size_t)1 << lg_n;
    bool cols;
    if (leaf_stride == 1 && col_stride >= n) cols = true;
    else if (col_stride == 1 && leaf_stride >= width) cols = false;
    else reject(who + ": strides are neither columns (leaf_stride == 1, col_stride >= n) nor rows (col_stride == 1, leaf_stride >= width)");
    const size_t last = checked_add(checked_mul(width - 1, col_stride, w, FRI_OVERFLOW), checked_mul(n - 1, leaf_stride, w, FRI_OVERFLOW), w, FRI_OVERFLOW);
    const size_t span = checked_mul(checked_add(last, 1, w, FRI_OVERFLOW), es, w, FRI_OVERFLOW);
    const size_t out_bytes = elems_bytes(n, sizeof(fr_t), w), w_bytes = elems_bytes(width, sizeof(fr_t), w);
    if ((uintptr_t)in % (es < 16 ? es : 16)) reject(who + ": misaligned in");
    if (ranges_meet(out, out_bytes, in, span)) reject(who + ": out may not overlap in");
    if (ranges_meet(out, out_bytes, weights, w_bytes)) reject(who + ": out may not overlap weights");
    if (sub != nullptr && ranges_meet(out, out_bytes, sub, sizeof(fr_t))) reject(who + ": sub may not overlap out");
    const gpu_info& gpu = select_gpu((int)device_id);

    call_scope sc(s);
#if defined(FEATURE_BABY_BEAR_X4)
    if (in_base) fri_reduce_run<bb31_dev>(gpu, sc, out, in, lg_n, width, col_stride, leaf_stride, cols, weights, sub, accumulate, s);
    else
#endif
    fri_reduce_run<fr_t>(gpu, sc, out, in, lg_n, width, col_stride, leaf_stride, cols, weights, sub, accumulate, s);
    sc.finish();
}
}

#ifdef SPPARK_FRI_HAS_DOMAIN
SPPARK_FFI RustError sppark_fri_fold(size_t device_id, void* out, const void* in, uint32_t lg_n, uint32_t lg_arity, const void* beta,
                                     const void* shift, int order, void* stream)
{   return guarded([&] { fri_fold_any(device_id, out, in, lg_n, lg_arity, beta, shift, order, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_fri_domain(size_t device_id, void* out, uint32_t lg_n, const void* shift, int order, const void* z, void* stream)
{   return guarded([&] { fri_domain_any(device_id, out, lg_n, shift, order, z, (hipStream_t)stream); });   }
#endif

SPPARK_FFI RustError sppark_fri_reduce(size_t device_id, void* out, const void* in, int in_base, uint32_t lg_n, size_t width,
                                       size_t col_stride, size_t leaf_stride, const void* weights, const void* sub, int accumulate,
                                       void* stream)
{
    return guarded([&] {
        fri_reduce_any(device_id, out, in, in_base, lg_n, width, col_stride, leaf_stride, weights, sub, accumulate, (hipStream_t)stream);
    });
}
