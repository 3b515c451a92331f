// HOST EMULATION TEST HARNESS for the NTT kernels (tests only; see emu_msm.cpp).
// Runs the phase functions of sppark_amd/csrc/ntt/ntt_kernels.hpp for every
// (tile, thread) the GPU grid would cover, over the steps of the driver's own route
// (sppark_amd/csrc/ntt/ntt_route.hpp make_ntt_route): no decision is made here.
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/ff/params.hpp"
#include "../../sppark_amd/csrc/ntt/ntt_kernels.hpp"
#include "../../sppark_amd/csrc/ntt/ntt_r64_kernels.hpp"
#include "../../sppark_amd/csrc/ntt/ntt_route.hpp"
#include "../../sppark_amd/csrc/ff/fr256_dev.hpp"
#include <vector>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
using namespace sppark_amd;

#if defined(FEATURE_GOLDILOCKS)
typedef gl64_dev F;
static F finv(F a) { return field_pow(a, (u64)F::MOD - 2); }
static F top_root() { return F::top_root(); }
static F group_gen() { return F::group_gen(); }
#elif defined(FEATURE_BABY_BEAR)
typedef bb31_dev F;
static F finv(F a) { return field_pow(a, (u64)F::MOD - 2); }
static F top_root() { return F::top_root(); }
static F group_gen() { return F::group_gen(); }
#else
# if defined(FEATURE_BLS12_381)
typedef bls12_381_fr_p FRP;
# else
typedef alt_bn128_fr_p FRP;
# endif
typedef fr256_dev<FRP> F;
static F pow_big(F b, const uint64_t* e, unsigned from_bit)
{
    F r = F::one();
    for (unsigned bit = from_bit; bit < 256; bit++) { if ((e[bit / 64] >> (bit % 64)) & 1) r = r * b; b = b * b; }
    return r;
}
static F finv(F a) { uint64_t e[4]; for (int i = 0; i < 4; i++) e[i] = FRP::MOD64[i]; e[0] -= 2; return pow_big(a, e, 0); }
static F group_gen() { F g = F::one(); F one = F::one(); for (unsigned i = 1; i < FRP::GROUP_GEN; i++) g = g + one; return g; }
static F top_root() { uint64_t e[4]; for (int i = 0; i < 4; i++) e[i] = FRP::MOD64[i]; e[0] -= 1; return pow_big(group_gen(), e, FRP::TWO_ADICITY); }
#endif


// ---- the knobs (ntt_route.hpp ntt_knobs; the driver's: ntt_engine::knobs()) and the hooks that set them ----
static const ntt_field g_field = ntt_field_of<F>();
static ntt_knobs g_knobs = ntt_default_knobs(g_field);
static bool g_no_r64 = false, g_no_scaled_table = false;    // ntt_call's refusals (the driver: a table the device had no room for)
extern "C" void emu_ntt_plan(unsigned r64_min, unsigned r64_direct) { g_knobs.r64_min = r64_min; g_knobs.r64_direct = r64_direct; }
extern "C" void emu_ntt_coset_fold(unsigned on) { g_knobs.coset_fold = on; }
// the one-stage-per-round passes (k_ntt_pass_lat): stages per pass (0: the register passes), log2 columns per tile row, log2
// tile elements (-1: the shape by size)
extern "C" void emu_ntt_lat(unsigned smax, int lgc, int lgtile) { g_knobs.lat_smax = smax; g_knobs.lat_lgc = lgc; g_knobs.lat_lgt = lgtile; }
extern "C" void emu_ntt_small(unsigned max_lg) { g_knobs.small_max = max_lg; }                    // 0 = the general path
extern "C" void emu_ntt_small_sized(unsigned on) { g_knobs.small_sized = on != 0; }               // 0: the run-time-size instance at every size
extern "C" void emu_ntt_refuse(unsigned no_r64, unsigned no_scaled_table) { g_no_r64 = no_r64 != 0; g_no_scaled_table = no_scaled_table != 0; }
// the plan of the one-stage-per-round passes for a size, the plan maker itself: out[4 * i ..] = {lg_cur, S, lgC, lgG} of
// pass i (GS order); returns the number of passes
extern "C" unsigned emu_ntt_lat_plan(unsigned lg, unsigned smax, int lgc, int lgtile, unsigned out[64])
{
    const ntt_plan pl = make_ntt_lat_plan(lg, smax, lgc, lgtile);
    for (unsigned i = 0; i < pl.npass && i < 16; i++) {
        out[4 * i] = pl.pass[i].lg_cur; out[4 * i + 1] = pl.pass[i].S; out[4 * i + 2] = pl.pass[i].lgC; out[4 * i + 3] = pl.pass[i].lgG;
    }
    return pl.npass;
}

// the knobs in force: {smax, lgc, lgt, r64_min, r64_direct, lat_smax, lat_lgc + 1, lat_lgt + 1, coset_fold, small_max, small_sized,
// packed_max, wide_table_lg, pass_table_max_lg}
extern "C" void emu_ntt_knobs(unsigned out[14])
{
    const ntt_knobs& k = g_knobs;
    const unsigned v[14] = {k.smax, k.lgc, k.lgt, k.r64_min, k.r64_direct, k.lat_smax, (unsigned)(k.lat_lgc + 1), (unsigned)(k.lat_lgt + 1), k.coset_fold,
                            k.small_max, k.small_sized, k.packed_max, k.wide_table_lg, k.pass_table_max_lg};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}

static ntt_call emu_call(unsigned lg, int order, int direction, int type)
{
    ntt_call c;
    c.lg = lg; c.order = order; c.direction = direction; c.type = type;
    c.no_r64 = g_no_r64; c.no_scaled_table = g_no_scaled_table;
    return c;
}
// how a coset transform of 2^lg elements runs: 0 separate scaling pass, 1 / 2 folded
extern "C" unsigned emu_ntt_coset_mode(unsigned lg, int order, int direction)
{   return make_ntt_route(g_field, g_knobs, emu_call(lg, order, direction, NTT_COSET)).cmode;   }

// ---- the route as integers (tests/test_ntt_route.py) ----
// call: {lg, order, direction, type, batch, col_stride, max_grid_y, aligned16, lde, lg_domain, lg_blowup, no_r64, no_scaled_table}
// out: {steps, tables, overflow, invalid, cols, gs, inverse, r64, cmode, lde_fused, step capacity, table capacity, launch_cols}, then
// per step {kernel, R1, R2, LGC, LG, gx, gy, block, lds, pass lg_cur, S, lgC, lgG, apply_scale, cmode, lg_cur, flags, bitrev,
//           tw, t1, t2, cz, crow, pass_tw (1 + the table's index, 0 = none), lde_src, lde_out, stages, scales}, then
// per table {family, kind, lg_cur, S, cmode, scaled, count, key family, key a, key b, key c}
// returns the words written, 0 when |cap| words do not hold the route
extern "C" unsigned emu_ntt_route(const unsigned call[13], unsigned* out, unsigned cap)
{
    ntt_call c;
    c.lg = call[0]; c.order = (int)call[1]; c.direction = (int)call[2]; c.type = (int)call[3]; c.batch = call[4]; c.col_stride = call[5];
    c.max_grid_y = call[6]; c.aligned16 = call[7] != 0; c.lde = (ntt_lde_mode)call[8]; c.lg_domain = call[9]; c.lg_blowup = call[10];
    c.no_r64 = call[11] != 0; c.no_scaled_table = call[12] != 0;
    const ntt_route r = make_ntt_route(g_field, g_knobs, c);
    if (cap < 13 + 28 * r.nsteps + 11 * r.ntables) return 0;
    unsigned* o = out;
    const unsigned head[13] = {r.nsteps, r.ntables, r.overflow, r.invalid, (unsigned)r.cols, r.gs, r.inverse, r.r64, r.cmode, r.lde_fused,
                               ntt_route::CAP, ntt_route::TCAP, (unsigned)ntt_launch_cols(g_knobs, c.lg, c.max_grid_y)};
    for (unsigned v : head) *o++ = v;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const ntt_step& s = r.steps[i];
        const unsigned v[28] = {s.kernel, s.R1, s.R2, s.LGC, s.LG, s.gx, s.gy, s.block, s.lds, s.pass.lg_cur, s.pass.S, s.pass.lgC, s.pass.lgG,
                                (unsigned)s.pass.apply_scale, s.pass.cmode, s.lg_cur, s.flags, (unsigned)s.bitrev, 1u + s.tw, 1u + s.t1, 1u + s.t2,
                                1u + s.cz, 1u + s.crow, 1u + s.pass_tw, s.lde_src, s.lde_out, s.stages, s.scales};
        for (unsigned x : v) *o++ = x;
    }
    for (unsigned i = 0; i < r.ntables; i++) {
        const ntt_table_req& q = r.tables[i];
        const unsigned v[11] = {q.family, q.kind, q.lg_cur, q.S, q.cmode, q.scaled, (unsigned)q.count, (unsigned)q.key_family, q.key_a, q.key_b, q.key_c};
        for (unsigned x : v) *o++ = x;
    }
    return (unsigned)(o - out);
}

// k_ntt_small keeps a butterfly pair per lane and swaps values between lanes (ntt_rx_xchg): here a work-group is |n|
// HOST THREADS, every exchange goes through the emulated LDS buffers, and the barrier hook of ntt_kernels.hpp is a counting
// barrier -- the product's own index math, twiddle choice, regrouping and permutations run unchanged (only ds_bpermute,
// the within-wave form of the exchange, is hardware-only: the GPU tests cover it).
namespace {
struct wg_barrier {
    std::mutex m; std::condition_variable cv;
    unsigned count = 0, gen = 0, n = 0;
    void wait()
    {
        std::unique_lock<std::mutex> lk(m);
        const unsigned g = gen;
        if (++count == n) { count = 0; gen++; cv.notify_all(); return; }
        cv.wait(lk, [&] { return gen != g; });
    }
} g_bar;
void run_group(unsigned n, const std::function<void(unsigned)>& body)
{
    g_bar.n = n; g_bar.count = 0;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < n; t++) th.emplace_back(body, t);
    for (auto& t : th) t.join();
}
} // namespace
extern "C" void sppark_emu_barrier() { g_bar.wait(); }

// ---- the tables of a transform size, from the kernels' own item functions ----
struct emu_tables {
    std::vector<F> lo, hi, glo, ghi, inner;
    ntt_tables<F> T, G;
    emu_tables(unsigned lg, bool inverse)
    {
        const unsigned h = lg < 12 ? lg : 12;
        lo.resize(1u << h); hi.resize((size_t)1 << (lg - h)); glo.resize(1u << h); ghi.resize((size_t)1 << (lg - h)); inner.resize(ntt_inner_entries<F>::value);
        F w = top_root();
        for (unsigned k = F::TWO_ADICITY; k > lg; k--) w = w * w;
        F g = group_gen();
        if (inverse) { w = finv(w); g = finv(g); }
        for (size_t k = 0; k < std::max<size_t>(std::max(lo.size(), hi.size()), inner.size()); k++) {
            table_item(lo.data(), hi.data(), inner.data(), w, lg, h, k);
            table_item(glo.data(), ghi.data(), (F*)nullptr, g, lg, h, k);
        }
        F two = F::one() + F::one();
        T = ntt_tables<F>{lo.data(), hi.data(), inner.data(), lg, h, finv(field_pow(two, lg))};
        G = ntt_tables<F>{glo.data(), ghi.data(), nullptr, lg, h, F::one()};
    }
};
// sppark_lde's hand-over (ntt_engine::lde_input): the compact coefficients and where the result goes
struct emu_lde_io { const F* src; unsigned lg_domain, lg_blowup; F* out; };

template<unsigned N> using uint_c = std::integral_constant<unsigned, N>;
template<class Fn> static void with_dif_inv(bool gs, bool inverse, Fn&& fn)
{
    if (gs) { if (inverse) fn(std::true_type(), std::true_type()); else fn(std::true_type(), std::false_type()); }
    else    { if (inverse) fn(std::false_type(), std::true_type()); else fn(std::false_type(), std::false_type()); }
}

// The steps of a route on the host: each kernel id by the loops over its phase functions, each table request by its item
// function.  One column (the packed kernel: |ncols| columns |stride| apart); |nt|: the lanes a pass's tile is run with.
static void emu_run_route(const ntt_route& r, F* d, unsigned lg, unsigned nt, const emu_lde_io& io = emu_lde_io{}, size_t ncols = 1, size_t stride = 0)
{
    const size_t n = (size_t)1 << lg;
    emu_tables tabs(lg, r.inverse);
    ntt_tables<F> T = tabs.T;
    const ntt_tables<F>& G = tabs.G;
    std::vector<std::vector<F>> tab(r.ntables);
    for (unsigned i = 0; i < r.ntables; i++) {
        const ntt_table_req& q = r.tables[i];
        tab[i].resize(q.count);
        for (size_t k = 0; k < q.count; k++)
            switch (q.family) {
                case NT_PASS: pass_table_item(tab[i].data(), T, q.lg_cur, q.S, k, (int)q.scaled); break;
                case NT_R64:  if constexpr (sizeof(F) <= 8) r64_table_item(tab[i].data(), T, q.kind, q.lg_cur, (int)q.scaled, k, q.cmode, &G); break;
                case NT_CZ:   if constexpr (sizeof(F) <= 8) r64_cz_item(tab[i].data(), G, q.cmode, (unsigned)k); break;
                case NT_CROW: pass_crow_item(tab[i].data(), G, q.cmode, q.S, (unsigned)k); break;
            }
    }
    auto t = [&](signed char k) { return k < 0 ? (const F*)nullptr : tab[k].data(); };
    with_dif_inv(r.gs, r.inverse, [&](auto DIF, auto INV) {
        constexpr bool dif = decltype(DIF)::value, inv = decltype(INV)::value;
        for (unsigned i = 0; i < r.nsteps; i++) {
            const ntt_step& s = r.steps[i];
            switch (s.kernel) {
            case NK_BITREV:
                for (size_t k = 0; k < n; k++) bitrev_item(d, lg, k);
                break;
            case NK_BITREV_TILED: case NK_BITREV_TILED_VEC: {      // the tile kernel's two phases
                constexpr unsigned TB = bitrev_tile_bits<F>::value;
                std::vector<F> lds(s.lds / sizeof(F));
                F* A = lds.data(); F* B = A + (((1u << TB) + 1) << TB);
                for (size_t mid = 0; mid < s.gx; mid++)
                    for (int phase = 0; phase < 2; phase++)
                        for (unsigned tid = 0; tid < s.block; tid++) {
                            if constexpr (sizeof(F) <= 8) {
                                if (s.kernel == NK_BITREV_TILED_VEC) { bitrev_tile_vec_item<F, TB>(d, A, B, lg, mid, tid, phase); continue; }
                            }
                            bitrev_tile_item<F, TB>(d, A, B, lg, mid, tid, s.block, phase);
                        }
                break;
            }
            case NK_COSET:
                for (size_t k = 0; k < n; k++) coset_item(d, G, s.bitrev, k);
                break;
            case NK_SMALL: {                                        // its lanes as host threads (the barrier hook above)
                std::vector<F> lds(2 * (size_t)s.block + 1);
                auto lane = [&](unsigned tid, auto LGC) {
                    constexpr unsigned C = sizeof(F) <= 8 ? decltype(LGC)::value : 0;      // (256-bit fields: the run-time form only)
                    if (s.flags & NTT_SMALL_GS) ntt_rx_run<F, inv, true, C>(d, lds.data(), T, G, s.flags, tid, s.block);
                    else                        ntt_rx_run<F, inv, false, C>(d, lds.data(), T, G, s.flags, tid, s.block);
                };
                run_group(s.block, [&](unsigned tid) {
                    switch (s.LGC) {
                        case 8:  lane(tid, uint_c<8>()); break;
                        case 9:  lane(tid, uint_c<9>()); break;
                        case 10: lane(tid, uint_c<10>()); break;
                        case 11: lane(tid, uint_c<11>()); break;
                        default: lane(tid, uint_c<0>()); break;
                    }
                });
                break;
            }
            case NK_SMALL_PACKED: {                                 // blockIdx.y: the kernel's own lane function, lanes as host threads
                std::vector<F> lds(2 * 256 + 1);
                for (size_t y = 0; y < s.gy; y++)
                    run_group(s.block, [&](unsigned tid) {
                        auto lane = [&](auto LG) { ntt_packed_lane<F, inv, decltype(LG)::value>(d, lds.data(), T, G, s.flags, stride, ncols, y, tid); };
                        switch (s.LG) {
                            case 1: lane(uint_c<1>()); break;
                            case 2: lane(uint_c<2>()); break;
                            case 3: lane(uint_c<3>()); break;
                            case 4: lane(uint_c<4>()); break;
                            case 5: lane(uint_c<5>()); break;
                            default: lane(uint_c<6>()); break;
                        }
                    });
                break;
            }
            case NK_PASS: case NK_PASS_LAT: {
                ntt_pass P = s.pass;
                P.crow = t(s.crow);
                if (r.r64) { P.cg_lo = G.lo; P.cg_hi = G.hi; P.cg_h = G.h; }
                T.pass_tw = t(s.pass_tw);
                const size_t tile_elems = (size_t)1 << (P.lgG + P.S + P.lgC);
                std::vector<F> tile(tile_elems + 1);
                for (size_t tile_id = 0; tile_id < s.gx; tile_id++) {
                    if (s.kernel == NK_PASS_LAT) {
                        for (unsigned tid = 0; tid < nt; tid++) ntt_lat_load<F, dif>(d, tile.data(), T, P, tile_id, tid, nt);
                        for (unsigned st = 0; st < P.S; st++)
                            for (unsigned tid = 0; tid < nt; tid++) ntt_lat_stage<F, dif, inv>(tile.data(), T, P, st, tid, nt);
                        for (unsigned tid = 0; tid < nt; tid++) ntt_lat_store<F, dif>(d, tile.data(), T, P, tile_id, tid, nt);
                        continue;
                    }
                    auto rounds = [&](auto R1, auto R2) {
                        constexpr unsigned r1 = decltype(R1)::value, r2 = decltype(R2)::value;
                        auto high = [&] { for (unsigned tid = 0; tid < nt; tid++) ntt_round_high<F, dif, inv, r1, r2>(d, tile.data(), T, P, tile_id, tid, nt); };
                        auto low = [&] { if (r2) for (unsigned tid = 0; tid < nt; tid++) ntt_round_low<F, dif, inv, r1, r2>(d, tile.data(), T, P, tile_id, tid, nt); };
                        if (dif) { high(); low(); } else { low(); high(); }
                    };
#define EMU_ROUNDS(R1, R2) rounds(uint_c<R1>(), uint_c<R2>())
                    SPPARK_NTT_DISPATCH_S(P.S, EMU_ROUNDS);
#undef EMU_ROUNDS
                }
                break;
            }
            case NK_NTT6: case NK_NTT12: case NK_NTT12_LDE:
                if constexpr (sizeof(F) <= 8) {
                    std::vector<F> tile(4096);
                    ntt_r64_args<F> A{T.inner, t(s.tw), t(s.t1), t(s.t2), s.lg_cur, t(s.cz)};
                    emu_tables dom(io.lg_domain, false);            // (NK_NTT12_LDE: the powers of g of the domain's size)
                    if (s.kernel == NK_NTT12_LDE) {
                        A.lde_src = io.src; A.lde_glo = dom.G.lo; A.lde_ghi = dom.G.hi; A.lde_gh = dom.G.h; A.lde_lgd = io.lg_domain; A.lde_lgb = io.lg_blowup;
                    }
                    for (size_t tile_id = 0; tile_id < s.gx; tile_id++) {
#define EMU_ALL(CALL) for (unsigned tid = 0; tid < s.block; tid++) { CALL; }
                        F* sub = d + (tile_id << 12);
                        if (s.kernel == NK_NTT6) {
                            if (dif) { EMU_ALL((ntt6_high<F, dif, inv>(d, tile.data(), A, tile_id, tid))) EMU_ALL((ntt6_low<F, dif, inv>(d, tile.data(), A, tile_id, tid))) }
                            else     { EMU_ALL((ntt6_low<F, dif, inv>(d, tile.data(), A, tile_id, tid))) EMU_ALL((ntt6_high<F, dif, inv>(d, tile.data(), A, tile_id, tid))) }
                        } else if (s.kernel == NK_NTT12_LDE) {      // k_ntt12<F, false, false, true>
                            EMU_ALL((ntt12_round<F, false, false, R12_B2, true>(sub, tile.data(), A, tid, tile_id)))
                            EMU_ALL((ntt12_round<F, false, false, R12_A2>(sub, tile.data(), A, tid))) EMU_ALL((ntt12_round<F, false, false, R12_B1>(sub, tile.data(), A, tid)))
                            EMU_ALL((ntt12_round<F, false, false, R12_A1>(sub, tile.data(), A, tid)))
                        } else if (dif) {
                            EMU_ALL((ntt12_round<F, dif, inv, R12_A1>(sub, tile.data(), A, tid))) EMU_ALL((ntt12_round<F, dif, inv, R12_B1>(sub, tile.data(), A, tid)))
                            EMU_ALL((ntt12_round<F, dif, inv, R12_A2>(sub, tile.data(), A, tid)))
                            // (ntt_r64_args::out: the last round stores to the LDE's output)
                            if (s.lde_out) { EMU_ALL((ntt12_round<F, dif, inv, R12_B2>(sub, tile.data(), A, tid, 0, io.out + (tile_id << 12)))) }
                            else           { EMU_ALL((ntt12_round<F, dif, inv, R12_B2>(sub, tile.data(), A, tid))) }
                        } else {
                            EMU_ALL((ntt12_round<F, dif, inv, R12_B2>(sub, tile.data(), A, tid))) EMU_ALL((ntt12_round<F, dif, inv, R12_A2>(sub, tile.data(), A, tid)))
                            EMU_ALL((ntt12_round<F, dif, inv, R12_B1>(sub, tile.data(), A, tid))) EMU_ALL((ntt12_round<F, dif, inv, R12_A1>(sub, tile.data(), A, tid)))
                        }
#undef EMU_ALL
                    }
                }
                break;
            case NK_LDE_SPREAD: {                                   // ntt_engine::lde_spread: lde_spread_item over every output element
                emu_tables dom(io.lg_domain, false);
                for (size_t o = 0; o < ((size_t)1 << (io.lg_domain + io.lg_blowup)); o++) lde_spread_item(d, io.src, dom.G, io.lg_domain, io.lg_blowup, 1, o);
                break;
            }
            case NK_COPY_OUT:
                memcpy((void*)io.out, (const void*)d, n * sizeof(F));
                break;
            default: break;
            }
        }
    });
}

static int emu_ntt_io(F* d, unsigned lg, ntt_call c, unsigned nt, const emu_lde_io& io, ntt_route* route = nullptr)
{
    c.aligned16 = ((uintptr_t)d & 15) == 0;
    const ntt_route r = make_ntt_route(g_field, g_knobs, c);
    if (route) *route = r;
    if (r.invalid || r.overflow) return -1;
    emu_run_route(r, d, lg, nt, io);
    return 0;
}
extern "C" int emu_ntt(void* inout, unsigned lg, int order, int direction, int type, unsigned nt)
{   return emu_ntt_io((F*)inout, lg, emu_call(lg, order, direction, type), nt, emu_lde_io{});   }

// ntt_engine::lde() with the kernel bodies run on the host: iNTT(NR) of the evaluations with its result handed to tmp,
// NTT(RN) of the extended buffer with the compact coefficients handed in.  Returns whether the spread was fused.
extern "C" int emu_lde(void* inout, unsigned lg_domain, unsigned lg_blowup, void* aux)
{
    F* ext = (F*)inout;
    const size_t dom = (size_t)1 << lg_domain, n_ext = dom << lg_blowup;
    std::vector<F> tmp(dom);
    ntt_call c = emu_call(lg_domain, NTT_NR, NTT_INVERSE, NTT_STANDARD);
    c.lde = NL_OUT;
    emu_ntt_io(ext, lg_domain, c, 64, emu_lde_io{nullptr, 0, 0, tmp.data()});
    if (aux) {
        for (size_t i = 0; i < dom; i++) {
            size_t r = 0;
            for (unsigned k = 0; k < lg_domain; k++) r |= ((i >> k) & 1) << (lg_domain - 1 - k);
            ((F*)aux)[r] = tmp[i];
        }
    }
    // (a fused spread never reads the extended buffer: filled with a pattern here)
    c = emu_call(lg_domain + lg_blowup, NTT_RN, NTT_FORWARD, NTT_STANDARD);
    c.lde = NL_SPREAD; c.lg_domain = lg_domain; c.lg_blowup = lg_blowup;
    if (make_ntt_route(g_field, g_knobs, c).lde_fused) memset((void*)ext, 0xA5, n_ext * sizeof(F));
    ntt_route r;
    emu_ntt_io(ext, lg_domain + lg_blowup, c, 64, emu_lde_io{tmp.data(), lg_domain, lg_blowup, nullptr}, &r);
    return r.lde_fused;
}
