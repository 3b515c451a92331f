// HOST EMULATION TEST HARNESS for the circle transform's kernels (tests only; see emu_ntt.cpp).
// Runs the phase functions of sppark_amd/csrc/circle/circle_kernels.hpp for every (tile, lane) the GPU grid would
// cover, over the steps of the driver's own route (circle_route.hpp make_circle_route): no decision is made here.
// A work-group's phases are separated by barriers on the GPU; here each phase runs for all lanes before the next.
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/ff/params.hpp"
#include "../../sppark_amd/csrc/circle/circle_kernels.hpp"
#include "../../sppark_amd/csrc/circle/circle_route.hpp"
#include <cstring>
#include <map>
#include <vector>
using namespace sppark_amd;

extern "C" void sppark_emu_barrier() {}

static circle_knobs g_knobs;
static unsigned g_max_grid_y = 65535;
static bool g_force_unaligned = false;
extern "C" void emu_circle_knobs(unsigned low_max, unsigned high_max, unsigned cache_max_lg, unsigned max_grid_y, unsigned unaligned)
{
    g_knobs = circle_knobs();
    if (low_max) g_knobs.low_max = low_max;
    if (high_max) g_knobs.high_max = high_max;
    if (cache_max_lg) g_knobs.cache_max_lg = cache_max_lg;
    g_max_grid_y = max_grid_y ? max_grid_y : 65535;
    g_force_unaligned = unaligned != 0;
}

static const circle_pt* points()
{
    static std::vector<circle_pt> pts;
    if (pts.empty()) { pts.resize(CIRCLE_PT_ENTRIES); for (unsigned i = 0; i < CIRCLE_PT_ENTRIES; i++) circle_point_item(pts.data(), i); }
    return pts.data();
}
static const cf_t* inv_table(unsigned m, bool y)
{
    static std::map<std::pair<unsigned, bool>, std::vector<cf_t>> tabs;
    auto& t = tabs[std::make_pair(m, y)];
    if (t.empty()) { t.resize((size_t)1 << (m - 2)); for (size_t h = 0; h < t.size(); h++) circle_inv_table_item(t.data(), points(), m, y ? 1 : 0, h); }
    return t.data();
}

static u32 scale_of(unsigned lg) { return lg == 0 ? 1u : 1u << (31 - lg); }

template<bool INV>
static void run_pass(cf_t* base, size_t stride, size_t cols, const circle_step& s, const circle_pass& P)
{
    std::vector<cf_t> lds(s.lds / sizeof(cf_t));               // exactly what the route asks the launch for
    cf_t* tw = lds.data() + circle_lds_elems(s.lgT);
    const unsigned nt = s.block;
    for (size_t y = 0; y < s.gy; y++)
        for (size_t tile = 0; tile < s.gx; tile++) {
            for (unsigned t = 0; t < nt; t++) circle_load(base, stride, cols, lds.data(), P, tile, y, t, nt);
            for (unsigned t = 0; t < nt; t++) circle_twiddles<INV>(tw, P, points(), tile, t, nt);
            const unsigned nr = circle_rounds(P.S);
            for (unsigned i = 0; i < nr; i++)
                for (unsigned t = 0; t < nt; t++) circle_round_at<INV>(lds.data(), tw, P, INV ? i : nr - 1 - i, t, nt);
            for (unsigned t = 0; t < nt; t++) circle_store(base, stride, cols, lds.data(), P, tile, y, t, nt);
        }
}

static int run(cf_t* d, unsigned lg, size_t batch, size_t stride, int order, int direction, unsigned pad_lg)
{
    if (lg == 0 || batch == 0) return 0;
    circle_call c;
    c.lg = lg; c.order = order; c.direction = direction; c.pad_lg = pad_lg; c.max_grid_y = g_max_grid_y;
    c.aligned16 = !g_force_unaligned && ((uintptr_t)d % 16 == 0) && (batch == 1 || stride % 4 == 0);
    for (size_t c0 = 0; c0 < batch; ) {
        c.batch = batch - c0;
        const circle_route r = make_circle_route(g_knobs, c);
        if (r.invalid || r.cols == 0) return -1;
        cf_t* base = d + c0 * stride;
        for (unsigned i = 0; i < r.nsteps; i++) {
            const circle_step& s = r.steps[i];
            if (s.kernel != CK_PASS) {                  // (the tiled variants: tests/emu/emu_ntt.cpp runs their phases)
                for (size_t col = 0; col < s.gy; col++)
                    for (size_t j = 0; j < ((size_t)1 << s.lg); j++) bitrev_item(base + col * stride, s.lg, j);
                continue;
            }
            circle_pass P;
            P.k = s.lg; P.b_lo = s.b_lo; P.S = s.S; P.lgC = s.lgC; P.lgT = s.lgT; P.vec = s.vec; P.pad_lg = s.pad_lg;
            P.scale = s.scales ? scale_of(s.lg) : 0;
            for (unsigned lb = 0; lb < CIRCLE_MAX_S; lb++)
                P.itw[lb] = s.table[lb] >= 0 ? inv_table(r.tables[s.table[lb]].m, r.tables[s.table[lb]].y) : nullptr;
            if (s.inverse) run_pass<true>(base, stride, r.cols, s, P); else run_pass<false>(base, stride, r.cols, s, P);
        }
        c0 += r.cols;
    }
    return 0;
}

extern "C" int emu_circle_ntt(uint32_t* data, unsigned lg, size_t batch, size_t stride, int order, int direction)
{   return run(reinterpret_cast<cf_t*>(data), lg, batch, stride ? stride : (size_t)1 << lg, order, direction, 32);   }

// the driver's LDE (circle_engine::lde): column j owns data[j * ext, (j + 1) * ext)
extern "C" int emu_circle_lde(uint32_t* data, unsigned lg, unsigned lg_blowup, size_t batch, int order, uint32_t* aux)
{
    cf_t* d = reinterpret_cast<cf_t*>(data);
    const size_t dom = (size_t)1 << lg, ext = (size_t)1 << (lg + lg_blowup);
    if (run(d, lg, batch, ext, order, CIRCLE_INVERSE, 32)) return -1;
    if (aux) for (size_t j = 0; j < batch; j++) memcpy(aux + j * dom, data + j * ext, dom * sizeof(uint32_t));
    return run(d, lg + lg_blowup, batch, ext, order, CIRCLE_FORWARD, lg_blowup ? lg : 32);
}

// ---- the route as integers (tests/test_circle_route.py) ----
// call: {lg, order, direction, batch, max_grid_y, aligned16, pad_lg}
// out: {nsteps, ntables, invalid, cols, scratch_entries, needs_points}, then per step {kernel, gx, gy, block, lds, lg, b_lo, S, lgC,
//       lgT, inverse, scales, vec, pad_lg}, then per table {m, y, cached, count}
extern "C" unsigned emu_circle_route(const uint64_t call[7], uint64_t* out, unsigned cap)
{
    circle_call c;
    c.lg = (unsigned)call[0]; c.order = (int)call[1]; c.direction = (int)call[2]; c.batch = (size_t)call[3];
    c.max_grid_y = (size_t)call[4]; c.aligned16 = call[5] != 0; c.pad_lg = (unsigned)call[6];
    const circle_route r = make_circle_route(g_knobs, c);
    if (cap < 6 + 14 * r.nsteps + 4 * r.ntables) return 0;
    uint64_t* o = out;
    *o++ = r.nsteps; *o++ = r.ntables; *o++ = r.invalid; *o++ = r.cols; *o++ = r.scratch_entries; *o++ = r.needs_points;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const circle_step& s = r.steps[i];
        const uint64_t v[14] = {s.kernel, s.gx, s.gy, s.block, s.lds, s.lg, s.b_lo, s.S, s.lgC, s.lgT, s.inverse, s.scales, s.vec, s.pad_lg};
        for (uint64_t x : v) *o++ = x;
    }
    for (unsigned i = 0; i < r.ntables; i++) {
        const circle_table_req& q = r.tables[i];
        *o++ = q.m; *o++ = q.y; *o++ = q.cached; *o++ = q.count;
    }
    return (unsigned)(o - out);
}
extern "C" unsigned emu_circle_point_entries() { return CIRCLE_PT_ENTRIES; }
