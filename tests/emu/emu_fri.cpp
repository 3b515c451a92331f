// HOST EMULATION TEST HARNESS for the FRI kernels (tests only; see emu_mle.cpp).
// Runs the per-lane functions of sppark_amd/csrc/fri/fri_kernels.hpp for every (work-group, lane) the GPU grid would cover,
// under the driver's own route (fri_route.hpp make_fri_route): no decision is made here.  The constants of the domain are
// formed with the field classes themselves (top_root(), inverse()), not with the driver's host arithmetic.
//
// Built once per field as a shared library for tests/test_emulation_fri.py and tests/test_fri_route.py.
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/ff/params.hpp"
#include "../../sppark_amd/csrc/ff/small_fields_dev.hpp"
#include "../../sppark_amd/csrc/ff/fr256_dev.hpp"
#include "../../sppark_amd/csrc/fri/fri_kernels.hpp"
#include <cstring>
#include <vector>
using namespace sppark_amd;

#if defined(FEATURE_GOLDILOCKS)
typedef gl64_dev F;
#elif defined(FEATURE_BABY_BEAR)
typedef bb31_dev F;
#elif defined(FEATURE_BABY_BEAR_X4)
typedef bb31_4_dev F;
#elif defined(FEATURE_MERSENNE31)
typedef mrs31_dev F;
#else
typedef fr256_dev<bls12_381_fr_p> F;
#endif
typedef fri_base<F>::type B;

extern "C" unsigned emu_fri_elem_bytes() { return (unsigned)sizeof(F); }
extern "C" unsigned emu_fri_tile_lg() { return fri_tile_lg(sizeof(F)); }
extern "C" unsigned emu_fri_red_chunk() { return FRI_RED_CHUNK; }
extern "C" unsigned emu_fri_lazy_terms() { return FRI_LAZY_TERMS; }

static unsigned g_wg_per_cu = FRI_WG_PER_CU;
extern "C" void emu_fri_set_wg_per_cu(unsigned v) { g_wg_per_cu = v; }

static fri_call call_of(const uint64_t c[9])
{
    fri_call k;
    k.elem_bytes = (size_t)c[0]; k.lg_n = (unsigned)c[1]; k.cus = (unsigned)c[2]; k.op = (int)c[3]; k.lg_arity = (unsigned)c[4];
    k.order = (int)c[5]; k.layout = (int)c[6]; k.width = (size_t)c[7]; k.aligned16 = c[8] != 0;
    return k;
}
// call: {elem_bytes, lg_n, cus, op, lg_arity, order, layout, width, aligned16}
// out: {invalid, grid, block, pack, acc, out_lg, tile_bits, grid_lg, tiles, chunks, vec}
extern "C" void emu_fri_route(const uint64_t call[9], uint64_t out[11])
{
    const fri_route r = make_fri_route(call_of(call));
    const uint64_t v[11] = {r.invalid, r.grid, r.block, r.pack, r.acc, r.out_lg, r.tile_bits, r.grid_lg, r.tiles, r.chunks, r.vec};
    memcpy(out, v, sizeof(v));
}

static bool aligned16(std::initializer_list<const void*> ps, int unaligned)
{
    uintptr_t all = 0;
    for (const void* p : ps) all |= (uintptr_t)p;
    return !unaligned && (all & 15) == 0;
}

#if !defined(FEATURE_MERSENNE31)
// the root of order 2^TWO_ADICITY: the single-word fields carry it; a 256-bit field's is gen^((r - 1) >> TWO_ADICITY)
template<class X> static X top_root_of(const X*) { return X::top_root(); }
template<class P> static fr256_dev<P> top_root_of(const fr256_dev<P>*)
{
    typedef fr256_dev<P> X;
    uint64_t e[P::N64];
    for (int i = 0; i < P::N64; i++) e[i] = P::MOD64[i];
    e[0] -= 1;
    X gen = X::one(), r = X::one();
    for (unsigned i = 1; i < P::GROUP_GEN; i++) gen = gen + X::one();
    for (unsigned bit = P::TWO_ADICITY; bit < 64 * P::N64; bit++) {
        if ((e[bit / 64] >> (bit % 64)) & 1) r = r * gen;
        gen = gen * gen;
    }
    return r;
}

template<unsigned CN>
static fri_consts<B, CN> consts_of(bool inverse, bool bitrev, const fri_geom& g, unsigned lg_n, unsigned lg_arity, const void* shift, unsigned pack)
{
    B w = top_root_of((const B*)nullptr);
    for (unsigned k = B::TWO_ADICITY; k > lg_n; k--) w = w * w;
    B sh = B::one();
    if (shift) memcpy(&sh, shift, sizeof(B));
    if (inverse) { w = w.inverse(); sh = sh.inverse(); }
    fri_consts<B, CN> k;
    k.base = sh;
    for (unsigned d = 0; d < 2; d++)                                // every entry by its definition, not digit by digit
        for (unsigned i = 0; i < 16; i++) k.tt[d][i] = field_pow(w, fri_lane_exp(bitrev, g, 0, i << (4 * d), pack));
    for (unsigned d = 0; d < 3; d++)
        for (unsigned i = 0; i < 16; i++) {
            const unsigned b = i << (4 * d);
            k.tb[d][i] = b >> g.grid_lg ? B::one() : field_pow(w, fri_lane_exp(bitrev, g, b, 0, pack));
        }
    k.step = field_pow(w, fri_step_exp(bitrev, g));
    k.scale = field_pow((B::one() + B::one()).inverse(), lg_arity);
    const B zeta = field_pow(w, (u64)1 << g.lg_m);
    for (unsigned t = 0; t < 4; t++) k.z[t] = lg_arity && t < (1u << (lg_arity - 1)) ? field_pow(zeta, fri_bitrev(t, lg_arity - 1)) : B::one();
    for (unsigned c = 0; c < CN; c++) k.c[c] = field_pow(w, fri_const_exp(bitrev, g, c / pack, c % pack, pack));
    return k;
}

static fri_route route_of(int op, unsigned lg_n, unsigned lg_arity, int order, unsigned cus, bool al, fri_geom& g)
{
    fri_call c;
    c.elem_bytes = sizeof(F); c.lg_n = lg_n; c.cus = cus; c.wg_per_cu = g_wg_per_cu; c.op = op; c.lg_arity = lg_arity; c.order = order; c.aligned16 = al;
    const fri_route r = make_fri_route(c);
    g = fri_geom{lg_n - (op == FRI_OP_FOLD ? lg_arity : 0), r.out_lg, r.tile_bits, r.grid_lg};
    return r;
}

template<unsigned LGA, bool BITREV, bool VEC>
static void fold_run(const fri_route& r, const fri_geom& g, F* out, const F* in, const F& beta, unsigned lg_n, const void* shift)
{
    typedef fri_fold_shape<F, LGA, VEC> S;
    if (r.pack != S::N || r.acc != S::U) abort();                  // the route and the kernel's shape agree
    const auto k = consts_of<S::CN>(true, BITREV, g, lg_n, LGA, shift, S::N);
    for (unsigned b = 0; b < r.grid; b++)
        for (unsigned t = 0; t < r.block; t++) fri_fold_lane<F, LGA, BITREV, VEC>(out, in, beta, k, g, b, t);
}
template<unsigned LGA>
static void fold_pick(const fri_route& r, const fri_geom& g, bool bitrev, F* out, const F* in, const F& beta, unsigned lg_n, const void* shift)
{
    const bool vec = sizeof(F) >= 16 || r.vec;
    if (vec) { if (bitrev) fold_run<LGA, true, true>(r, g, out, in, beta, lg_n, shift); else fold_run<LGA, false, true>(r, g, out, in, beta, lg_n, shift); }
    else     { if (bitrev) fold_run<LGA, true, false>(r, g, out, in, beta, lg_n, shift); else fold_run<LGA, false, false>(r, g, out, in, beta, lg_n, shift); }
}
extern "C" int emu_fri_fold(void* out, const void* in, unsigned lg_n, unsigned lg_arity, const void* beta, const void* shift, int order,
                            unsigned cus, int unaligned)
{
    fri_geom g;
    const fri_route r = route_of(FRI_OP_FOLD, lg_n, lg_arity, order, cus, aligned16({out, in}, unaligned), g);
    if (r.invalid) return -1;
    const bool bitrev = order == FRI_BITREV;
    if (lg_arity == 1)      fold_pick<1>(r, g, bitrev, (F*)out, (const F*)in, *(const F*)beta, lg_n, shift);
    else if (lg_arity == 2) fold_pick<2>(r, g, bitrev, (F*)out, (const F*)in, *(const F*)beta, lg_n, shift);
    else                    fold_pick<3>(r, g, bitrev, (F*)out, (const F*)in, *(const F*)beta, lg_n, shift);
    return 0;
}

template<bool BITREV, bool VEC>
static void domain_run(const fri_route& r, const fri_geom& g, F* out, const F& z, unsigned lg_n, const void* shift)
{
    typedef fri_domain_shape<F, VEC> S;
    if (r.pack != S::N || r.acc != S::U) abort();
    const auto k = consts_of<S::CN>(false, BITREV, g, lg_n, 0, shift, S::N);
    for (unsigned b = 0; b < r.grid; b++)
        for (unsigned t = 0; t < r.block; t++) fri_domain_lane<F, BITREV, VEC>(out, z, k, g, b, t);
}
extern "C" int emu_fri_domain(void* out, unsigned lg_n, const void* shift, int order, const void* z, unsigned cus, int unaligned)
{
    fri_geom g;
    const fri_route r = route_of(FRI_OP_DOMAIN, lg_n, 0, order, cus, aligned16({out}, unaligned), g);
    if (r.invalid) return -1;
    F zv = mle_zero<F>();
    if (z) memcpy(&zv, z, sizeof(F));
    const bool vec = sizeof(F) >= 16 || r.vec, bitrev = order == FRI_BITREV;
    if (vec) { if (bitrev) domain_run<true, true>(r, g, (F*)out, zv, lg_n, shift); else domain_run<false, true>(r, g, (F*)out, zv, lg_n, shift); }
    else     { if (bitrev) domain_run<true, false>(r, g, (F*)out, zv, lg_n, shift); else domain_run<false, false>(r, g, (F*)out, zv, lg_n, shift); }
    return 0;
}
#endif

template<class E, bool COLS, bool VEC>
static void reduce_run(const fri_route& r, F* out, const E* in, const F* w, size_t n, size_t width, size_t cs, size_t ls, const F& sub, int accumulate)
{
    for (unsigned b = 0; b < r.grid; b++)                           // a work-group walks the chunks itself, as the kernel does
        for (size_t j0 = 0; j0 < width; j0 += FRI_RED_CHUNK) {
            const unsigned cw = (unsigned)(width - j0 < FRI_RED_CHUNK ? width - j0 : FRI_RED_CHUNK);
            for (unsigned t = 0; t < r.block; t++)
                fri_reduce_lane<F, E, COLS, VEC>(out, in, w + j0, n, j0, cw, cs, ls, sub, j0 == 0, accumulate != 0, b, r.grid, t);
        }
}
template<class E>
static int reduce_any(void* out, const void* in, unsigned lg_n, size_t width, size_t cs, size_t ls, const void* weights, const void* sub,
                      int accumulate, unsigned cus, int unaligned)
{
    const size_t n = (size_t)1 << lg_n;
    const bool cols = ls == 1 && cs >= n;
    if (!cols && !(cs == 1 && ls >= width)) return -1;
    fri_call c;
    c.elem_bytes = sizeof(E); c.lg_n = lg_n; c.cus = cus; c.wg_per_cu = g_wg_per_cu; c.op = FRI_OP_REDUCE; c.layout = cols ? FRI_COLUMNS : FRI_ROWS; c.width = width;
    c.aligned16 = aligned16({in}, unaligned) && (((cols ? cs : ls) * sizeof(E)) & 15) == 0;
    const fri_route r = make_fri_route(c);
    if (r.invalid || r.chunks != (width + FRI_RED_CHUNK - 1) / FRI_RED_CHUNK) return -1;
    F sv = mle_zero<F>();
    if (sub) memcpy(&sv, sub, sizeof(F));
    const bool vec = sizeof(E) >= 16 || r.vec;
    if (vec && cols && r.pack != fri_pack(sizeof(E))) return -1;
    if (cols) { if (vec) reduce_run<E, true, true>(r, (F*)out, (const E*)in, (const F*)weights, n, width, cs, ls, sv, accumulate);
                else     reduce_run<E, true, false>(r, (F*)out, (const E*)in, (const F*)weights, n, width, cs, ls, sv, accumulate); }
    else      { if (vec) reduce_run<E, false, true>(r, (F*)out, (const E*)in, (const F*)weights, n, width, cs, ls, sv, accumulate);
                else     reduce_run<E, false, false>(r, (F*)out, (const E*)in, (const F*)weights, n, width, cs, ls, sv, accumulate); }
    return 0;
}
extern "C" int emu_fri_reduce(void* out, const void* in, int in_base, unsigned lg_n, size_t width, size_t cs, size_t ls, const void* weights,
                              const void* sub, int accumulate, unsigned cus, int unaligned)
{
#if defined(FEATURE_BABY_BEAR_X4)
    if (in_base) return reduce_any<bb31_dev>(out, in, lg_n, width, cs, ls, weights, sub, accumulate, cus, unaligned);
#endif
    if (in_base) return -1;
    return reduce_any<F>(out, in, lg_n, width, cs, ls, weights, sub, accumulate, cus, unaligned);
}
