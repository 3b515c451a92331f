// HOST EMULATION TEST HARNESS for the multilinear-table kernels (tests only; see emu_ntt.cpp).
// Runs the phase functions of sppark_amd/csrc/mle/mle_kernels.hpp for every (work-group, lane) the GPU grid would cover, over
// the steps of the driver's own route (mle_route.hpp make_mle_route): no decision is made here.  A lane exchange of the GPU
// is a phase of its own here: every lane's value is kept, then every lane combines its own with its partner's.
//
// Built once per field as a shared library for tests/test_emulation_mle.py and tests/test_mle_route.py, and with
// -DEMU_MLE_MAIN as a stand-alone program that checks itself against plain loops (for a sanitizer run).
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/ff/params.hpp"
#include "../../sppark_amd/csrc/ff/small_fields_dev.hpp"
#include "../../sppark_amd/csrc/ff/fr256_dev.hpp"
#include "../../sppark_amd/csrc/mle/mle_kernels.hpp"
#include <cstdio>
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

static mle_route route_of(unsigned lg_n, int op, unsigned rows, unsigned cus, bool aligned16)
{
    mle_call c;
    c.elem_bytes = sizeof(F); c.lg_n = lg_n; c.cus = cus; c.op = op; c.rows = rows; c.aligned16 = aligned16;
    return make_mle_route(c);
}
static bool aligned16(std::initializer_list<const void*> ps, int unaligned)
{
    uintptr_t all = 0;
    for (const void* p : ps) all |= (uintptr_t)p;
    return !unaligned && (all & 15) == 0;
}
static bool use_vec(const mle_step& s) { return sizeof(F) >= 16 || s.vec; }

extern "C" unsigned emu_mle_elem_bytes() { return (unsigned)sizeof(F); }
extern "C" unsigned emu_mle_tile_lg() { return mle_geom<F>::T; }

// ---- the route as integers (tests/test_mle_route.py) ----
// call: {elem_bytes, lg_n, cus, op, rows, aligned16}
// out: {nsteps, invalid, scratch_elems}, then per step {kernel, grid, block, tile_lg, vars, var_base, tiles, writes, vec}
extern "C" unsigned emu_mle_route(const uint64_t call[6], uint64_t* out, unsigned cap)
{
    mle_call c;
    c.elem_bytes = (size_t)call[0]; c.lg_n = (unsigned)call[1]; c.cus = (unsigned)call[2]; c.op = (int)call[3]; c.rows = (unsigned)call[4];
    c.aligned16 = call[5] != 0;
    const mle_route r = make_mle_route(c);
    if (cap < 3 + 9 * r.nsteps) return 0;
    uint64_t* o = out;
    *o++ = r.nsteps; *o++ = r.invalid; *o++ = r.scratch_elems;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const mle_step& s = r.steps[i];
        const uint64_t v[9] = {s.kernel, s.grid, s.block, s.tile_lg, s.vars, s.var_base, s.tiles, s.writes, s.vec};
        for (uint64_t x : v) *o++ = x;
    }
    return (unsigned)(o - out);
}

// ---- fold ----
template<bool HIGH>
static void fold_run(const mle_step& s, F* out, const F* in, const F& r, size_t half)
{
    for (unsigned b = 0; b < s.grid; b++)
        for (unsigned t = 0; t < s.block; t++) {
            if (use_vec(s)) mle_fold_lane<F, HIGH, true>(out, in, r, half, b, s.grid, t);
            else            mle_fold_lane<F, HIGH, false>(out, in, r, half, b, s.grid, t);
        }
}
extern "C" int emu_mle_fold(void* out, const void* in, unsigned lg_n, const void* r, int order, unsigned cus, int unaligned)
{
    const mle_route rt = route_of(lg_n, MLE_OP_FOLD, 0, cus, aligned16({out, in}, unaligned));
    if (rt.invalid || rt.nsteps != 1 || rt.steps[0].kernel != MK_FOLD) return -1;
    const size_t half = (size_t)1 << (lg_n - 1);
    if (order == MLE_HIGH) fold_run<true>(rt.steps[0], (F*)out, (const F*)in, *(const F*)r, half);
    else                   fold_run<false>(rt.steps[0], (F*)out, (const F*)in, *(const F*)r, half);
    return 0;
}

// ---- evaluate ----
template<bool VEC>
static void bind_run(const mle_step& s, F* out, const F* in, const F* pt)
{
    std::vector<F> v(s.block), nxt(s.block);
    for (unsigned b = 0; b < s.grid; b++)
        for (size_t tile = b; tile < s.tiles; tile += s.grid) {
            for (unsigned t = 0; t < s.block; t++) v[t] = mle_bind_lane<F, VEC>(in, tile, s.tile_lg, pt, t);
            for (unsigned e = 0; e < 6; e++) {
                const unsigned bit = mle_lane_bit<F, VEC>(e);
                if (bit >= s.tile_lg) break;
                for (unsigned t = 0; t < s.block; t++) nxt[t] = mle_bind_pair(v[t], v[t ^ (1u << e)], (t >> e) & 1, pt[bit]);
                v.swap(nxt);
            }
            F w[MLE_NT / 64];
            for (unsigned k = 0; k < MLE_NT / 64; k++) w[k] = v[64 * k];
            out[tile] = mle_bind_waves<F, VEC>(w, s.tile_lg, pt);
        }
}
extern "C" int emu_mle_evaluate(void* ret, const void* in, unsigned lg_n, const void* point, unsigned cus, int unaligned)
{
    if (lg_n == 0) { memcpy(ret, in, sizeof(F)); return 0; }
    const mle_route rt = route_of(lg_n, MLE_OP_EVALUATE, 0, cus, aligned16({in}, unaligned));
    if (rt.invalid || rt.nsteps == 0) return -1;
    std::vector<F> scratch(rt.scratch_elems);                   // exactly what the route asks for
    F* slot = scratch.data();
    const F* src = (const F*)in;
    unsigned bound = 0;
    for (unsigned i = 0; i < rt.nsteps; i++) {
        const mle_step& s = rt.steps[i];
        if (s.kernel != MK_BIND || s.var_base != bound) return -1;
        if (use_vec(s)) bind_run<true>(s, slot, src, (const F*)point + s.var_base);
        else            bind_run<false>(s, slot, src, (const F*)point + s.var_base);
        src = slot; slot += s.writes; bound += s.vars;
    }
    if (bound != lg_n || slot != scratch.data() + rt.scratch_elems) return -1;
    memcpy(ret, src, sizeof(F));
    return 0;
}

// ---- eq ----
template<bool VEC>
static void eq_run(const mle_step& s, F* out, const F* point, unsigned lg_n)
{
    constexpr unsigned N = VEC ? mle_geom<F>::PACK : 1, U = mle_geom<F>::E / N;
    const unsigned tl = s.tile_lg, nhigh = lg_n - tl, steps = mle_eq_steps(nhigh);
    std::vector<F> pre(s.block), nxt(s.block);
    for (unsigned b = 0; b < s.grid; b++) {
        std::vector<mle_chunk<F, N>> X((size_t)s.block * U);
        for (unsigned t = 0; t < s.block; t++) mle_eq_lane<F, VEC>(&X[(size_t)t * U], point, tl, t);
        for (size_t tile = b; tile < s.tiles; tile += s.grid) {
            for (unsigned t = 0; t < s.block; t++) {
                const unsigned l = t & ((1u << steps) - 1);
                F p = F::one(), q = F::one();
                if (l < nhigh) { p = point[tl + l]; q = F::one() - p; }
                pre[t] = mle_eq_factor(p, q, nhigh, tile, l);
            }
            for (unsigned e = 0; e < steps; e++) {
                for (unsigned t = 0; t < s.block; t++) nxt[t] = pre[t] * pre[t ^ (1u << e)];
                pre.swap(nxt);
            }
            for (unsigned t = 0; t < s.block; t++) mle_eq_store<F, VEC>(out, &X[(size_t)t * U], pre[t], nhigh, tile, tl, t);
        }
    }
}
extern "C" int emu_mle_eq(void* out, const void* point, unsigned lg_n, unsigned cus, int unaligned)
{
    const mle_route rt = route_of(lg_n, MLE_OP_EQ, 0, cus, aligned16({out}, unaligned));
    if (rt.invalid || rt.nsteps != 1 || rt.steps[0].kernel != MK_EQ || rt.steps[0].vars != lg_n) return -1;
    if (use_vec(rt.steps[0])) eq_run<true>(rt.steps[0], (F*)out, (const F*)point, lg_n);
    else                      eq_run<false>(rt.steps[0], (F*)out, (const F*)point, lg_n);
    return 0;
}

// ---- round ----
template<int NTAB, int FORM, bool HIGH, bool VEC>
static void round_run(const mle_step& s, F* slab, const mle_tables<F>& tabs, size_t half)
{
    constexpr unsigned ROWS = sumcheck_shape<NTAB, FORM>::ROWS;
    for (unsigned b = 0; b < s.grid; b++) {
        F row[ROWS];
        for (unsigned c = 0; c < ROWS; c++) row[c] = mle_zero<F>();
        for (unsigned t = 0; t < s.block; t++) {
            F acc[ROWS];
            sumcheck_round_lane<F, NTAB, FORM, HIGH, VEC>(acc, tabs, half, b, s.grid, t);
            for (unsigned c = 0; c < ROWS; c++) row[c] = row[c] + acc[c];
        }
        for (unsigned c = 0; c < ROWS; c++) slab[(size_t)b * ROWS + c] = row[c];
    }
}
template<int NTAB, int FORM>
static void round_pick(const mle_step& s, F* slab, const mle_tables<F>& tabs, size_t half, int order)
{
    const bool vec = use_vec(s);
    if (order == MLE_HIGH) { if (vec) round_run<NTAB, FORM, true, true>(s, slab, tabs, half); else round_run<NTAB, FORM, true, false>(s, slab, tabs, half); }
    else                   { if (vec) round_run<NTAB, FORM, false, true>(s, slab, tabs, half); else round_run<NTAB, FORM, false, false>(s, slab, tabs, half); }
}
extern "C" int emu_mle_round(void* out, const void* const* tables, unsigned ntables, int form, unsigned lg_n, int order, unsigned cus,
                             int unaligned)
{
    if (ntables < 1 || ntables > SUMCHECK_MAX_TABLES || (form == SUMCHECK_EQ_MUL_SUB && ntables != 4)) return -1;
    const unsigned rows = form == SUMCHECK_EQ_MUL_SUB ? 4 : ntables + 1;
    mle_tables<F> tabs;
    bool al = true;
    for (unsigned k = 0; k < SUMCHECK_MAX_TABLES; k++) {
        tabs.p[k] = (const F*)tables[k < ntables ? k : 0];
        al = al && aligned16({tabs.p[k]}, unaligned);
    }
    const mle_route rt = route_of(lg_n, MLE_OP_ROUND, rows, cus, al);
    if (rt.invalid || rt.nsteps != 2 || rt.steps[0].kernel != MK_ROUND || rt.steps[1].kernel != MK_ROUND_SUM) return -1;
    if (rt.steps[0].writes != (size_t)rt.steps[0].grid * rows || rt.steps[1].tiles != rt.steps[0].grid || rt.steps[1].grid != 1) return -1;
    std::vector<F> scratch(rt.scratch_elems);
    F* slab = scratch.data();
    const size_t half = (size_t)1 << (lg_n - 1);
    const mle_step& s = rt.steps[0];
    if (form == SUMCHECK_EQ_MUL_SUB) round_pick<4, SUMCHECK_EQ_MUL_SUB>(s, slab, tabs, half, order);
    else if (ntables == 1) round_pick<1, SUMCHECK_PRODUCT>(s, slab, tabs, half, order);
    else if (ntables == 2) round_pick<2, SUMCHECK_PRODUCT>(s, slab, tabs, half, order);
    else if (ntables == 3) round_pick<3, SUMCHECK_PRODUCT>(s, slab, tabs, half, order);
    else                   round_pick<4, SUMCHECK_PRODUCT>(s, slab, tabs, half, order);
    F* sums = slab + s.writes;
    for (unsigned c = 0; c < rows; c++) sums[c] = mle_zero<F>();
    for (unsigned t = 0; t < rt.steps[1].block; t++) {
        F acc[SUMCHECK_MAX_ROWS];
        sumcheck_sum_lane(acc, slab, rt.steps[1].tiles, rows, t);
        for (unsigned c = 0; c < rows; c++) sums[c] = sums[c] + acc[c];
    }
    memcpy(out, sums, rows * sizeof(F));
    return 0;
}

#ifdef EMU_MLE_MAIN
// Stand-alone self-check: every operation at every size up to T + 2 against plain loops over the same field class.
static uint64_t g_seed = 0x9e3779b97f4a7c15ULL;
static uint64_t next64() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }
static F rnd() { F x = F::one(), y = F::one(); for (int i = 0; i < 8; i++) { x = x + x; if (next64() & 1) x = x + y; y = y * x + F::one(); } return y * x; }
static bool same(const F& a, const F& b) { return memcmp(&a, &b, sizeof(F)) == 0; }

int main()
{
    const unsigned T = mle_geom<F>::T, cus = 3;
    int bad = 0;
    for (unsigned lg = 0; lg <= T + 2; lg++) {
        const size_t n = (size_t)1 << lg, half = n / 2;
        std::vector<F> tab[4], point(lg ? lg : 1);
        for (auto& tb : tab) { tb.resize(n); for (auto& x : tb) x = rnd(); }
        for (auto& x : point) x = rnd();
        for (int unaligned = 0; unaligned < 2; unaligned++) {
            // evaluate against eq, eq against the definition
            std::vector<F> eq(n), want(n);
            if (emu_mle_eq(eq.data(), point.data(), lg, cus, unaligned)) bad++;
            for (size_t i = 0; i < n; i++) {
                F w = F::one();
                for (unsigned j = 0; j < lg; j++) w = w * (((i >> j) & 1) ? point[j] : F::one() - point[j]);
                if (!same(w, eq[i])) { bad++; break; }
            }
            F ev, dot = mle_zero<F>();
            if (emu_mle_evaluate(&ev, tab[0].data(), lg, point.data(), cus, unaligned)) bad++;
            for (size_t i = 0; i < n; i++) dot = dot + tab[0][i] * eq[i];
            if (!same(ev, dot)) bad++;
            if (lg == 0) continue;
            for (int order = 0; order < 2; order++) {
                std::vector<F> out(half);
                const F r = point[0];
                if (emu_mle_fold(out.data(), tab[0].data(), lg, &r, order, cus, unaligned)) bad++;
                for (size_t i = 0; i < half; i++) {
                    const F lo = order ? tab[0][i] : tab[0][2 * i], hi = order ? tab[0][i + half] : tab[0][2 * i + 1];
                    if (!same(out[i], lo + r * (hi - lo))) { bad++; break; }
                }
                for (unsigned shape = 1; shape <= 5; shape++) {
                    const unsigned nt = shape == 5 ? 4 : shape, rows = shape == 5 ? 4 : nt + 1;
                    const int form = shape == 5 ? SUMCHECK_EQ_MUL_SUB : SUMCHECK_PRODUCT;
                    const void* ptr[4] = {tab[0].data(), tab[1].data(), tab[2].data(), tab[3].data()};
                    F got[SUMCHECK_MAX_ROWS], ref[SUMCHECK_MAX_ROWS];
                    if (emu_mle_round(got, ptr, nt, form, lg, order, cus, unaligned)) bad++;
                    for (unsigned c = 0; c < rows; c++) ref[c] = mle_zero<F>();
                    for (size_t i = 0; i < half; i++) {
                        F f[4], d[4];
                        for (unsigned k = 0; k < nt; k++) {
                            const F lo = order ? tab[k][i] : tab[k][2 * i], hi = order ? tab[k][i + half] : tab[k][2 * i + 1];
                            f[k] = lo; d[k] = hi - lo;
                        }
                        for (unsigned c = 0; c < rows; c++) {
                            F term = f[0];
                            if (form == SUMCHECK_EQ_MUL_SUB) term = f[0] * (f[1] * f[2] - f[3]);
                            else for (unsigned k = 1; k < nt; k++) term = term * f[k];
                            ref[c] = ref[c] + term;
                            for (unsigned k = 0; k < nt; k++) f[k] = f[k] + d[k];
                        }
                    }
                    for (unsigned c = 0; c < rows; c++) if (!same(got[c], ref[c])) bad++;
                }
            }
        }
    }
    printf("emu_mle self-check, %u-byte elements, lg_n 0 .. %u: %s (%d mismatches)\n", (unsigned)sizeof(F), T + 2, bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
#endif
