// Host driver of the NTT: the role of the reference's NTT class + NTTParameters
// (ntt/ntt.cuh:31-366, ntt/parameters.cuh:222-337): order/direction/type
// dispatch, per-(device, size, direction) twiddle tables built once on the
// device and kept for the life of the process, kernel sequence on one stream.
// WHAT runs is decided in ntt_route.hpp (make_ntt_route: a pure function); run() here fetches the tables a route asks
// for and launches its steps.
#pragma once
#include "ntt_kernels.hpp"
#include "ntt_r64_kernels.hpp"
#include "ntt_route.hpp"
#include "../ff/fr256_dev.hpp"
#include "../ff/mont_host.hpp"
#include "../util/runtime.hpp"
#include <map>
#include <mutex>
#include <tuple>

namespace sppark_amd {

// ---- host-side constants (parameter setup only; no transform code here) ------
template<class F> struct host_field;
template<> struct host_field<gl64_dev> {
    typedef unsigned __int128 u128;
    static u64 mul(u64 a, u64 b) { return (u64)(((u128)a * b) % gl64_dev::MOD); }
    static u64 pow(u64 b, u64 e) { u64 r = 1; while (e) { if (e & 1) r = mul(r, b); b = mul(b, b); e >>= 1; } return r; }
    static u64 inv(u64 a) { return pow(a, gl64_dev::MOD - 2); }
    static u64 top_root() { return gl64_dev::TOP_ROOT; }
    static u64 gen() { return gl64_dev::GROUP_GEN; }
    static u64 two_pow(unsigned lg) { return pow(2, lg); }
    static gl64_dev wire(u64 canonical) { gl64_dev r; r.v = canonical; return r; }
};
template<> struct host_field<bb31_dev> {                        // canonical arithmetic, converted at the end
    static constexpr u64 P = bb31_dev::MOD;
    static u64 mul(u64 a, u64 b) { return a * b % P; }
    static u64 pow(u64 b, u64 e) { u64 r = 1; while (e) { if (e & 1) r = mul(r, b); b = mul(b, b); e >>= 1; } return r; }
    static u64 inv(u64 a) { return pow(a, P - 2); }
    static u64 top_root() { return mul(bb31_dev::TOP_ROOT, inv((1ULL << 32) % P)); }   // out of Montgomery form
    static u64 gen() { return bb31_dev::GROUP_GEN; }
    static u64 two_pow(unsigned lg) { return pow(2, lg); }
    static bb31_dev wire(u64 canonical) { bb31_dev r; r.v = (u32)((canonical << 32) % P); return r; }
};

// 256-bit fields: everything stays in the Montgomery domain, which is the wire format
template<class P> struct host_field<fr256_dev<P>> {
    typedef mont_host<P> H;
    struct elem { H v; };
    static elem mul(const elem& a, const elem& b) { return elem{a.v * b.v}; }
    static elem one() { return elem{H::one()}; }
    static elem small(unsigned k) { elem r{H::zero()}; for (unsigned i = 0; i < k; i++) r.v = r.v + H::one(); return r; }
    static elem inv(const elem& a) { return elem{a.v.inverse()}; }
    static elem gen() { return small(P::GROUP_GEN); }
    static elem top_root()                          // gen^((r-1) >> S)
    {
        uint64_t e[P::N64];
        for (int i = 0; i < P::N64; i++) e[i] = P::MOD64[i];
        e[0] -= 1;                                  // r is odd
        elem r = one(), b = gen();
        for (unsigned bit = P::TWO_ADICITY; bit < 64 * P::N64; bit++) {
            if ((e[bit / 64] >> (bit % 64)) & 1) r = mul(r, b);
            // square AFTER use: b = gen^(2^(bit - S + 1))
            b = mul(b, b);
        }
        return r;
    }
    static elem two_pow(unsigned lg) { elem r = one(), two = small(2); for (unsigned i = 0; i < lg; i++) r = mul(r, two); return r; }
    static fr256_dev<P> wire(const elem& a) { fr256_dev<P> r; memcpy(r.v, a.v.v, sizeof(r.v)); return r; }
};

template<class F>
class ntt_engine {
    struct table_set { F *lo, *hi, *inner, *glo, *ghi; unsigned h; F scale; };
    // Inter-pass twiddle tables, keyed (device, direction) + the key of the route's table request (ntt_route.hpp
    // ntt_table_req: shared by every transform size unless the table carries 1/n or coset powers).  (Round 3 kept one copy
    // per (size, direction): a forward + inverse 2^24 transform of a 256-bit field pinned > 1.1 GB, and more for every
    // further size.)
    typedef std::tuple<int, int, int, unsigned, unsigned, unsigned> tw_key;
    std::map<tw_key, F*> tw_cache;
    static constexpr bool R64 = sizeof(F) <= 8;                    // the radix-64 plan's kernels exist (ntt_r64_kernels.hpp)
    std::map<std::tuple<int, unsigned, int>, table_set> cache;     // (hip device, lg, inverse)
    std::mutex mtx;
    template<unsigned N> using uint_c = std::integral_constant<unsigned, N>;

    // The plan's shape parameters (ntt_route.hpp ntt_knobs).  A shipped library uses the defaults; a tuning build
    // (-DSPPARK_TUNING, e.g. SPPARK_EXTRA_FLAGS=-DSPPARK_TUNING python -m sppark_amd.build; tools/gpu_ntt_sweep.py) reads
    // them from the environment once per process.  The LDS tile is clamped to what the element size allows (160 KB per
    // work-group: 2^14 eight-byte elements, 2^12 32-byte ones; the one-stage-per-round passes stay within the
    // 64 KB a launch gets without raising the kernel's limit).
    static const ntt_knobs& knobs()
    {
        static const ntt_knobs knobs = [] {
            const ntt_field f = ntt_field_of<F>();
            ntt_knobs k = ntt_default_knobs(f);
#ifdef SPPARK_TUNING
            const unsigned S_MAX = k.smax;
            // 256-bit fields: stages per one-stage-per-round pass (0: the register passes), columns per tile row and tile
            // elements (log2; default: by size, make_ntt_lat_plan)
            if (const char* e = getenv("SPPARK_NTT_LAT_SMAX")) { unsigned v = (unsigned)atoi(e); if (v <= 8) k.lat_smax = R64 ? 0 : v; }
            if (const char* e = getenv("SPPARK_NTT_LAT_LGC")) { int v = atoi(e); if (v >= 0 && v <= 3) k.lat_lgc = v; }
            if (const char* e = getenv("SPPARK_NTT_LAT_LGTILE")) { int v = atoi(e); if (v >= 6 && v <= 11) k.lat_lgt = v; }
            if (const char* e = getenv("SPPARK_NTT_COSET_FOLD")) k.coset_fold = (unsigned)atoi(e);    // 0: the separate scaling launch
            if (const char* e = getenv("SPPARK_NTT_R64_MIN")) k.r64_min = (unsigned)atoi(e);          // 99: the 8-stage plan only
            if (const char* e = getenv("SPPARK_NTT_R64_DIRECT")) k.r64_direct = (unsigned)atoi(e);    // largest single inter-pass table (log2)
            if (const char* e = getenv("SPPARK_NTT_SMAX")) { unsigned v = (unsigned)atoi(e); if (v >= 1 && v <= S_MAX) k.smax = v; }
            if (const char* e = getenv("SPPARK_NTT_LGC")) { unsigned v = (unsigned)atoi(e); if (v >= 1 && v <= 8) k.lgc = v; }
            if (const char* e = getenv("SPPARK_NTT_LGTILE")) {
                unsigned v = (unsigned)atoi(e), cap = 17;
                while (((size_t)sizeof(F) << cap) > 160 * 1024) cap--;
                if (v >= 8 && v <= cap) k.lgt = v;
            }
            if (const char* e = getenv("SPPARK_NTT_WIDE_TABLE")) k.wide_table_lg = (unsigned)atoi(e);                    // 0 = no tables
            if (const char* e = getenv("SPPARK_NTT_SMALL_MAX")) k.small_max = std::min((unsigned)atoi(e), f.small_cap);    // 0 = never
            if (const char* e = getenv("SPPARK_NTT_PACKED_MAX")) k.packed_max = std::min((unsigned)atoi(e), NTT_PACKED_MAX_LG);   // 0 = never
            if (const char* e = getenv("SPPARK_NTT_SMALL_SIZED")) k.small_sized = atoi(e) != 0;    // 0: the run-time-size instance at every size
#endif
            if (k.lgt < k.smax + 1) k.lgt = k.smax + 1;
            return k;
        }();
        return knobs;
    }
    // Find or build one table.  The engine lock is NOT held while the table is allocated, generated and synchronised
    // (another thread's transform of a cached size goes on meanwhile); two threads that miss the same key both build
    // it and the loser frees its copy.  Returns nullptr when the device has no room for it -- the idle scratch buffers
    // are given back first -- and the caller falls back to a plan without that table.
    template<class Launch>
    const F* cached_table(const tw_key& key, size_t count, hipStream_t stream, Launch&& launch)
    {
        {
            std::lock_guard<std::mutex> lk(mtx);
            auto it = tw_cache.find(key);
            if (it != tw_cache.end()) return it->second;
        }
        F* tw = nullptr;
        hipError_t e = dev_scratch_pool::malloc_or_drain((void**)&tw, count * sizeof(F));
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return nullptr; }
        HIP_OK(e);
        launch(tw);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);      // visible to every later call on any stream
        if (e != hipSuccess) { (void)hipFree(tw); HIP_OK(e); }
        std::lock_guard<std::mutex> lk(mtx);
        auto ins = tw_cache.emplace(key, tw);
        if (!ins.second) (void)hipFree(tw);                         // built twice: keep the first
        return ins.first->second;
    }

    // one table of a route (ntt_route.hpp ntt_table_req), found in the cache or built by its kernel; G: the powers of the
    // coset generator
    const F* route_table(int hip_dev, int inverse, const ntt_table_req& q, const ntt_tables<F>& T, const ntt_tables<F>& G, hipStream_t stream)
    {
        const unsigned grid = (unsigned)((q.count + 255) / 256);
        return cached_table(tw_key(hip_dev, inverse, q.key_family, q.key_a, q.key_b, q.key_c), q.count, stream, [&](F* t) {
            switch (q.family) {
                case NT_PASS: hipLaunchKernelGGL(k_pass_table<F>, dim3(grid), dim3(256), 0, stream, t, T, q.lg_cur, q.S, (int)q.scaled); break;
                case NT_R64:  hipLaunchKernelGGL(k_r64_table<F>, dim3(grid), dim3(256), 0, stream, t, T, q.kind, q.lg_cur, (int)q.scaled, q.cmode, G); break;
                case NT_CZ:   hipLaunchKernelGGL(k_r64_cz<F>, dim3(1), dim3(64), 0, stream, t, G, q.cmode); break;
                case NT_CROW: hipLaunchKernelGGL(k_pass_crow<F>, dim3(1), dim3(256), 0, stream, t, G, q.cmode, q.S); break;
            }
        });
    }

    // (gs, inverse) -> the DIF and INV template arguments of the transform kernels, as compile-time constants
    template<class Fn> static void with_dif_inv(bool gs, bool inverse, Fn&& fn)
    {
        if (gs) { if (inverse) fn(std::true_type(), std::true_type()); else fn(std::true_type(), std::false_type()); }
        else    { if (inverse) fn(std::false_type(), std::true_type()); else fn(std::false_type(), std::false_type()); }
    }
    static void launch_bitrev(const ntt_step& s, F* d, unsigned lg, size_t col_stride, hipStream_t stream)
    {
        constexpr unsigned TB = bitrev_tile_bits<F>::value;
        const dim3 grid(s.gx, s.gy), block(s.block);
        if (s.kernel == NK_BITREV) hipLaunchKernelGGL(k_bitrev<F>, grid, block, 0, stream, d, lg, col_stride);
        else if (s.kernel == NK_BITREV_TILED) hipLaunchKernelGGL((k_bitrev_tiled<F, TB>), grid, block, s.lds, stream, d, lg, col_stride);
        else if constexpr (sizeof(F) <= 8) hipLaunchKernelGGL((k_bitrev_tiled_vec<F, TB>), grid, block, s.lds, stream, d, lg, col_stride);
    }

    table_set tables(int hip_dev, unsigned lg, int inverse, hipStream_t stream)
    {
        std::lock_guard<std::mutex> lk(mtx);
        auto key = std::make_tuple(hip_dev, lg, inverse);
        auto it = cache.find(key);
        if (it != cache.end()) return it->second;
        typedef host_field<F> H;
        table_set t;
        t.h = lg < 12 ? lg : 12;
        size_t nlo = (size_t)1 << t.h, nhi = (size_t)1 << (lg - t.h);
        HIP_OK(dev_scratch_pool::malloc_or_drain((void**)&t.lo, (2 * (nlo + nhi) + ntt_inner_entries<F>::value) * sizeof(F)));
        t.hi = t.lo + nlo; t.glo = t.hi + nhi; t.ghi = t.glo + nlo; t.inner = t.ghi + nhi;
        auto w = H::top_root();
        for (unsigned k = F::TWO_ADICITY; k > lg; k--) w = H::mul(w, w);
        auto g = H::gen();
        if (inverse) { w = H::inv(w); g = H::inv(g); }
        t.scale = H::wire(H::inv(H::two_pow(lg)));
        unsigned grid = (unsigned)((std::max<size_t>(std::max(nlo, nhi), ntt_inner_entries<F>::value) + 255) / 256);
        hipLaunchKernelGGL(k_tables<F>, dim3(grid), dim3(256), 0, stream, t.lo, t.hi, t.inner, H::wire(w), lg, t.h);
        hipLaunchKernelGGL(k_tables<F>, dim3(grid), dim3(256), 0, stream, t.glo, t.ghi, (F*)nullptr, H::wire(g), lg, t.h);
        HIP_OK(hipGetLastError());
        // one-time: the tables are shared by every later call on ANY stream, so they must be
        // complete before another thread can find them in the cache
        HIP_OK(hipStreamSynchronize(stream));
        return cache.emplace(key, t).first->second;
    }

public:
    static ntt_engine& instance() { static ntt_engine e; return e; }

    // Free every cached table of this library (sppark_ntt_release_cached); they are rebuilt on demand.  The caller
    // guarantees that no transform of this library is in flight.
    void release_tables()
    {
        std::lock_guard<std::mutex> lk(mtx);
        int cur = 0; (void)hipGetDevice(&cur);
        for (auto& kv : tw_cache) { (void)hipSetDevice(std::get<0>(kv.first)); (void)hipFree(kv.second); }
        for (auto& kv : cache) { (void)hipSetDevice(std::get<0>(kv.first)); (void)hipFree(kv.second.lo); }
        tw_cache.clear(); cache.clear();
        (void)hipSetDevice(cur);
    }
    size_t cached_table_count() { std::lock_guard<std::mutex> lk(mtx); return tw_cache.size() + cache.size(); }

    // in-place transform of a DEVICE buffer of 2^lg elements on |stream|
    // |lde| (sppark_lde's forward RN transform only): the input is still the COMPACT coefficients lde->src (2^lg_domain, bit-reversed
    // order, unshifted); the first step of the radix-64 plan reads them as the spread array (k_ntt12<.., LDE>), and where the
    // transform runs another plan the spread is a step of its own in front.
    // |lde->out| instead (sppark_lde's inverse NR transform): the result goes to |out|, |d| is scratch afterwards -- the last step
    // of the radix-64 plan stores there (ntt_r64_args::out), any other plan runs in place and copies.
    // |batch| columns (sppark_ntt_batch / sppark_lde_batch): column j at d + j * col_stride.  Every launch takes one grid
    // row per column (blockIdx.y; the packed kernel: one per work-group of columns) and the columns share the tables; lde->src
    // and lde->out then hold the columns packed, 2^lde->lg_domain and 2^lg elements apart.  A batch above what one launch can
    // index (launch_cols) runs as several launch chunks, each with a route of its own.
    struct lde_input { const F* src; unsigned lg_domain, lg_blowup; F* out; };
    void run(const gpu_info& gpu, F* d, unsigned lg, int order, int direction, int type, hipStream_t stream, const lde_input* lde = nullptr,
             size_t batch = 1, size_t col_stride = 0)
    {
        ntt_call call;
        call.lg = lg; call.order = order; call.direction = direction; call.type = type;
        call.col_stride = col_stride; call.max_grid_y = (size_t)std::max(gpu.prop.maxGridSize[1], 1);
        if (lde) { call.lde = lde->out ? NL_OUT : NL_SPREAD; call.lg_domain = lde->lg_domain; call.lg_blowup = lde->lg_blowup; }
        const size_t per = launch_cols(gpu, lg);
        for (size_t c0 = 0; c0 < batch; c0 += per) {
            call.batch = std::min(per, batch - c0);
            F* dc = d + c0 * col_stride;
            call.aligned16 = ((uintptr_t)dc & 15) == 0 && (call.batch == 1 || ((col_stride * sizeof(F)) & 15) == 0);
            lde_input sub{};
            if (lde) { sub = *lde; if (sub.src) sub.src += c0 << lde->lg_domain; if (sub.out) sub.out += c0 << lg; }
            run_chunk(gpu, dc, call, sub, stream);
        }
    }

private:
    // one launch chunk: route, tables, launches
    void run_chunk(const gpu_info& gpu, F* d, ntt_call call, const lde_input& lde, hipStream_t stream)
    {
        const ntt_field fld = ntt_field_of<F>();
        const unsigned lg = call.lg;
        const size_t n = (size_t)1 << lg, col_stride = call.col_stride;
        ntt_route r = make_ntt_route(fld, knobs(), call);
        if (r.invalid || r.overflow) HIP_OK(hipErrorInvalidValue);
        ntt_tables<F> T{}, G{};
        const F* tab[ntt_route::TCAP] = {};
        if (lg) {
            const table_set ts = tables(gpu.hip_id, lg, r.inverse, stream);
            T = ntt_tables<F>{ts.lo, ts.hi, ts.inner, lg, ts.h, ts.scale, nullptr}; G = ntt_tables<F>{ts.glo, ts.ghi, nullptr, lg, ts.h, ts.scale, nullptr};
            // The tables, fetched (first call: built) BEFORE anything is launched.  If the device has no room for one of
            // the radix-64 plan's, the transform runs the 8-stage plan, whose passes can generate their twiddles; if it has
            // none for the table that carries 1/n, the shared unscaled one (or none) and the last pass multiplies by 1/n
            // itself; without an unscaled inter-pass table a pass generates its twiddles.
            for (unsigned i = 0; i < r.ntables; i++) {
                const ntt_table_req& q = r.tables[i];
                if ((tab[i] = route_table(gpu.hip_id, r.inverse, q, T, G, stream)) != nullptr || (q.family == NT_PASS && !q.scaled)) continue;
                if (q.family == NT_PASS) call.no_scaled_table = true; else call.no_r64 = true;
                r = make_ntt_route(fld, knobs(), call);
                i = ~0u;                                            // (again from the first table of the new route)
            }
        }
        const size_t cols = r.cols;
        with_dif_inv(r.gs, r.inverse, [&](auto DIF, auto INV) {
            constexpr bool dif = decltype(DIF)::value, inv = decltype(INV)::value;
            for (unsigned i = 0; i < r.nsteps; i++) {
                const ntt_step& s = r.steps[i];
                const dim3 grid(s.gx, s.gy), block(s.block);
                auto t = [&](signed char k) { return k < 0 ? (const F*)nullptr : tab[k]; };
                switch (s.kernel) {
                case NK_BITREV: case NK_BITREV_TILED: case NK_BITREV_TILED_VEC:
                    launch_bitrev(s, d, lg, col_stride, stream);
                    break;
                case NK_COSET:
                    hipLaunchKernelGGL(k_coset<F>, grid, block, 0, stream, d, G, s.bitrev, col_stride);
                    break;
                case NK_SMALL: {
                    auto go = [&](auto LGC) {
                        hipLaunchKernelGGL((k_ntt_small<F, inv, decltype(LGC)::value>), grid, block, s.lds, stream, d, T, G, s.flags, col_stride);
                    };
                    if constexpr (sizeof(F) <= 8) {
                        switch (s.LGC) {
                            case 8:  go(uint_c<8>()); break;
                            case 9:  go(uint_c<9>()); break;
                            case 10: go(uint_c<10>()); break;
                            case 11: go(uint_c<11>()); break;
                            default: go(uint_c<0>()); break;
                        }
                    } else
                        go(uint_c<0>());
                    break;
                }
                case NK_SMALL_PACKED: {
                    auto go = [&](auto LG) {
                        hipLaunchKernelGGL((k_ntt_small_packed<F, inv, decltype(LG)::value>), grid, block, 0, stream, d, T, G, s.flags, col_stride, cols);
                    };
                    switch (s.LG) {
                        case 1: go(uint_c<1>()); break;
                        case 2: go(uint_c<2>()); break;
                        case 3: go(uint_c<3>()); break;
                        case 4: go(uint_c<4>()); break;
                        case 5: go(uint_c<5>()); break;
                        default: go(uint_c<6>()); break;
                    }
                    break;
                }
                case NK_PASS: case NK_PASS_LAT: {
                    ntt_pass P = s.pass;
                    P.crow = t(s.crow);
                    if (r.r64) { P.cg_lo = G.lo; P.cg_hi = G.hi; P.cg_h = G.h; }        // (a folded coset transform)
                    T.pass_tw = t(s.pass_tw);
                    if (s.kernel == NK_PASS_LAT) {
                        if constexpr (!R64) hipLaunchKernelGGL((k_ntt_pass_lat<F, dif, inv>), grid, block, s.lds, stream, d, T, P, col_stride);
                        break;
                    }
                    auto go = [&](auto R1, auto R2) {
                        auto* fn = k_ntt_pass<F, dif, inv, decltype(R1)::value, decltype(R2)::value>;
                        if (s.lds > 65536) HIP_OK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
                        hipLaunchKernelGGL(fn, grid, block, s.lds, stream, d, T, P, col_stride);
                    };
#define SPPARK_NTT_GO(R1, R2) go(uint_c<R1>(), uint_c<R2>())
                    if constexpr (sizeof(F) <= 8) { SPPARK_NTT_DISPATCH_S(P.S, SPPARK_NTT_GO); }       // (the instances that exist: k_ntt_pass.hip)
                    else                          { SPPARK_NTT_DISPATCH_S4(P.S, SPPARK_NTT_GO); }
#undef SPPARK_NTT_GO
                    break;
                }
                case NK_NTT6: case NK_NTT12: case NK_NTT12_LDE:
                    if constexpr (R64) {
                        ntt_r64_args<F> A{T.inner, t(s.tw), t(s.t1), t(s.t2), s.lg_cur, t(s.cz)};
                        if (s.lde_out) { A.out = lde.out; A.aux_stride = n; }
                        if (s.kernel == NK_NTT12_LDE) {
                            const table_set tg = tables(gpu.hip_id, lde.lg_domain, 0, stream);
                            A.lde_src = lde.src; A.lde_glo = tg.glo; A.lde_ghi = tg.ghi; A.lde_gh = tg.h;
                            A.lde_lgd = lde.lg_domain; A.lde_lgb = lde.lg_blowup; A.aux_stride = (size_t)1 << lde.lg_domain;
                            hipLaunchKernelGGL((k_ntt12<F, false, false, true>), grid, block, s.lds, stream, d, A, col_stride);
                        } else if (s.kernel == NK_NTT6) hipLaunchKernelGGL((k_ntt6<F, dif, inv>), grid, block, s.lds, stream, d, A, col_stride);
                        else hipLaunchKernelGGL((k_ntt12<F, dif, inv>), grid, block, s.lds, stream, d, A, col_stride);
                    }
                    break;
                case NK_LDE_SPREAD:
                    lde_spread(gpu, d, lde.src, lde.lg_domain, lde.lg_blowup, true, stream, cols, col_stride, s.spread_in_stride);
                    break;
                case NK_COPY_OUT:
                    copy_cols(lde.out, n, d, col_stride, n, cols, stream);
                    break;
                default: break;
                }
            }
        });
        HIP_OK(hipGetLastError());
    }

public:
    // columns one launch of run() covers (ntt_route.hpp ntt_launch_cols)
    size_t launch_cols(const gpu_info& gpu, unsigned lg)
    {   return ntt_launch_cols(knobs(), lg, (size_t)std::max(gpu.prop.maxGridSize[1], 1));   }
    // |batch| columns of |n| elements from src (src_stride apart) to dst (dst_stride apart), device to device
    static void copy_cols(F* dst, size_t dst_stride, const F* src, size_t src_stride, size_t n, size_t batch, hipStream_t stream)
    {
        if (batch == 1) HIP_OK(hipMemcpyAsync(dst, src, n * sizeof(F), hipMemcpyDeviceToDevice, stream));
        else HIP_OK(hipMemcpy2DAsync(dst, dst_stride * sizeof(F), src, src_stride * sizeof(F), n * sizeof(F), batch, hipMemcpyDeviceToDevice, stream));
    }

    // in-place bit-reversal permutation (NN and RR orders; ntt/ntt.cuh:44-79): 16-byte accesses for the single-word fields
    // where every column starts 16-byte aligned (ntt_route.hpp ntt_route_bitrev)
    static void bit_reverse(F* d, unsigned lg, hipStream_t stream, size_t batch = 1, size_t col_stride = 0)
    {
        const bool aligned16 = ((uintptr_t)d & 15) == 0 && (batch == 1 || ((col_stride * sizeof(F)) & 15) == 0);
        launch_bitrev(ntt_route_bitrev(ntt_field_of<F>(), lg, batch, aligned16), d, lg, col_stride, stream);
    }

    // d_inout[idx] *= g^(rev(idx))   (NTT::LDE_powers(stream, d_inout, lg), ntt/ntt.cuh:352-356)
    void lde_powers(const gpu_info& gpu, F* d, unsigned lg, hipStream_t stream)
    {
        if (lg > F::TWO_ADICITY) HIP_OK(hipErrorInvalidValue);
        const table_set ts = tables(gpu.hip_id, lg, 0, stream);
        ntt_tables<F> G{ts.glo, ts.ghi, nullptr, lg, ts.h, ts.scale, nullptr};
        const size_t n = (size_t)1 << lg;
        hipLaunchKernelGGL(k_coset<F>, dim3((unsigned)std::min<size_t>((n + 255) / 256, (size_t)1 << 22)), dim3(256), 0, stream, d, G, 1, (size_t)0);
        HIP_OK(hipGetLastError());
    }

    // d_out[idx << lg_blowup] = d_in[idx] (* g^rev(idx) when |shift|), zeros elsewhere
    // (NTT::LDE_expand / LDE_launch, ntt/ntt.cuh:247-281,358-365).  The buffers either do not overlap or
    // d_in is aligned to the END of d_out ("d_out is expected to encompass d_in and d_in is expected to be
    // aligned to the end of d_out", ntt.cuh:358-360; any other overlap is an error, as the reference's
    // assert, ntt/kernels.cu:176).  In place: output o needs input o >> lg_blowup, which sits at position
    // P(o) = ext - dom + (o >> lg_blowup) >= o, so an output range [lo, hi) may be written in one launch
    // as long as P(lo) >= hi: hi = ext - (ext - lo) / blowup.  The ranges shrink geometrically
    // ([0, ext - dom), then dom (1 - 1/blowup) elements, ...): 2 + lg_domain / lg_blowup launches, kernel
    // boundaries instead of the reference's cooperative grid sync (kernels.cu:199-200).
    // |batch| > 1 (run() within the batched LDE): separate buffers, the columns out_stride / in_stride elements apart
    void lde_spread(const gpu_info& gpu, F* d_out, const F* d_in, unsigned lg_domain, unsigned lg_blowup,
                    bool shift, hipStream_t stream, size_t batch = 1, size_t out_stride = 0, size_t in_stride = 0)
    {
        if (lg_domain + lg_blowup > F::TWO_ADICITY) HIP_OK(hipErrorInvalidValue);
        const size_t dom = (size_t)1 << lg_domain, ext = dom << lg_blowup;
        const bool overlap = (d_in < d_out + ext) && (d_out < d_in + dom);
        if (overlap && (lg_blowup == 0 || d_in != d_out + (ext - dom))) HIP_OK(hipErrorInvalidValue);
        const table_set ts = tables(gpu.hip_id, lg_domain, 0, stream);
        ntt_tables<F> G{ts.glo, ts.ghi, nullptr, lg_domain, ts.h, ts.scale, nullptr};
        // (a grid row per column: more columns than the grid's y dimension -- the packed sizes' launch chunks hold up to
        //  256 / (n/2) times as many -- take several launches)
        const size_t rows = (size_t)std::max(gpu.prop.maxGridSize[1], 1);
        for (size_t c0 = 0; c0 < batch; c0 += rows) {
            const unsigned ncol = (unsigned)std::min(rows, batch - c0);
            for (size_t lo = 0; lo < ext;) {
                const size_t hi = overlap ? ext - ((ext - lo) >> lg_blowup) : ext;
                hipLaunchKernelGGL(k_lde_spread<F>, dim3((unsigned)((hi - lo + 255) / 256), ncol), dim3(256), 0, stream,
                                   d_out + c0 * out_stride, d_in + c0 * in_stride, G, lg_domain, lg_blowup, (int)shift, lo, hi, out_stride, in_stride);
                lo = hi;
            }
        }
        HIP_OK(hipGetLastError());
    }

    // Low-degree extension on the coset g*H' (NTT::LDE_aux, ntt/ntt.cuh:283-336):
    // iNTT(NR) of the 2^lg_domain evaluations in d_ext[0 .. 2^lg_domain), coset shift +
    // zero-extension in bit-reversed order, forward NTT(RN) of size 2^(lg_domain+lg_blowup).
    // d_tmp: 2^lg_domain scratch elements; d_aux (nullable): the coefficients, natural order.
    // |batch| columns (sppark_lde_batch): d_ext's 2^(lg_domain + lg_blowup) elements apart, d_tmp's and d_aux's packed.
    void lde(const gpu_info& gpu, F* d_ext, F* d_tmp, F* d_aux, unsigned lg_domain, unsigned lg_blowup, hipStream_t stream, size_t batch = 1)
    {
        if (lg_domain + lg_blowup > F::TWO_ADICITY) HIP_OK(hipErrorInvalidValue);
        const size_t dom = (size_t)1 << lg_domain, ext = dom << lg_blowup;
        // (the inverse transform runs in the first 2^lg_domain elements of d_ext -- overwritten below anyway -- and leaves the
        //  coefficients in d_tmp: its last step stores there, no copy in front of it)
        const lde_input lo{nullptr, 0, 0, d_tmp};
        run(gpu, d_ext, lg_domain, NTT_NR, NTT_INVERSE, NTT_STANDARD, stream, &lo, batch, ext);
        if (d_aux) {
            const size_t rows = (size_t)std::max(gpu.prop.maxGridSize[1], 1);
            for (size_t c0 = 0; c0 < batch; c0 += rows)
                hipLaunchKernelGGL(k_bitrev_copy<F>, dim3((unsigned)((dom + 255) / 256), (unsigned)std::min(rows, batch - c0)), dim3(256), 0, stream,
                                   d_aux + c0 * dom, d_tmp + c0 * dom, lg_domain, dom);
            HIP_OK(hipGetLastError());
        }
        // (the spread + coset shift of LDE_launch ride in the forward transform's first step where the plan allows: 134 MB
        //  never written and a launch less at 2^22 -> 2^24)
        const lde_input li{d_tmp, lg_domain, lg_blowup, nullptr};
        run(gpu, d_ext, lg_domain + lg_blowup, NTT_RN, NTT_FORWARD, NTT_STANDARD, stream, &li, batch, ext);
    }
};

} // namespace sppark_amd
