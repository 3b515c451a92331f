// HOST TEST HARNESS (tests only): the plan of an MSM (sppark_amd/csrc/msm/msm_plan.hpp) for the host, so that its
// invariants -- what the kernels' launch shapes and LDS sizes rely on -- can be checked over every size in the GPU-less
// container (tests/test_plan.py), and the route -- the sequence of launches -- that msm_route.hpp makes of it
// (tests/test_msm_route.py).
#include "../../sppark_amd/csrc/msm/msm_route.hpp"
using namespace sppark_amd;

static void put(const msm_plan& p, unsigned out[21])
{
    const unsigned v[21] = {p.n, p.wbits, p.nwins, p.NB, p.nbits, p.HB, p.LB, p.NA, p.L, p.chunks_per_win, p.nslabs, p.slab_sz,
                            p.F, p.K, p.K1, p.G, p.wpg, p.big, p.IB, p.SH, p.NG};
    for (int i = 0; i < 21; i++) out[i] = v[i];
}
// out: {n, wbits, nwins, NB, nbits, HB, LB, NA, L, chunks_per_win, nslabs, slab_sz, F, K, K1, G, wpg, big, IB, SH, NG}
extern "C" void emu_make_plan(size_t npoints, unsigned scalar_bits, unsigned wbits, unsigned L, unsigned F, unsigned K,
                              unsigned nslabs, unsigned LB, unsigned groups, unsigned K1, unsigned records, unsigned out[21])
{
    msm_tunables t;
    t.wbits = wbits; t.L = L; t.F = F; t.K = K; t.nslabs = nslabs; t.LB = LB; t.groups = groups; t.K1 = K1; t.records = records;
    put(make_plan(npoints, scalar_bits, t), out);
}
// the automatic plan as the driver asks for it: with the device's resident k_accumulate lanes known
extern "C" void emu_make_plan_resident(size_t npoints, unsigned scalar_bits, size_t resident_lanes, unsigned out[21])
{
    msm_tunables t;
    t.resident_lanes = resident_lanes;
    put(make_plan(npoints, scalar_bits, t), out);
}
extern "C" void emu_make_fixed_plan(size_t npoints, unsigned fb_wbits, unsigned fb_nwins, unsigned register_stage, unsigned out[21])
{
    msm_tunables t;
    put(make_fixed_plan(npoints, fb_wbits, fb_nwins, register_stage, t), out);
}

// ---- the route (sppark_amd/csrc/msm/msm_route.hpp): the launch sequence of an MSM as flat integers ----
// tun: {wbits, L, F, K, nslabs, LB, groups, K1, records, top, tail code, g2 path, long_runs}
static bool tunables(const unsigned tun[13], size_t resident_lanes, msm_tunables& t)
{
    t.wbits = tun[0]; t.L = tun[1]; t.F = tun[2]; t.K = tun[3]; t.nslabs = tun[4]; t.LB = tun[5]; t.groups = tun[6]; t.K1 = tun[7];
    t.records = tun[8]; t.top = tun[9]; t.g2_coop = tun[11]; t.long_runs = tun[12]; t.resident_lanes = resident_lanes;
    return decode_tail_code(tun[10], t.sw);
}
// the plan under all the tunables the route reads too; 0: the tail code is refused
extern "C" int emu_make_plan_tuned(size_t npoints, unsigned scalar_bits, const unsigned tun[13], size_t resident_lanes, unsigned out[21])
{
    msm_tunables t;
    if (!tunables(tun, resident_lanes, t)) return 0;
    put(make_plan(npoints, scalar_bits, t), out);
    return 1;
}
// out: {no_join, no_narrow_end, no_latency_sums, no_coop, no_piece_tree, convert_per_lane, top_per_sum, piece_level_launches,
//       sums_one_lane, piece_fuse_max (two words)}; 0: refused
extern "C" int emu_decode_tail_code(unsigned code, unsigned out[11])
{
    msm_switches s;
    const bool ok = decode_tail_code(code, s);
    const unsigned v[11] = {s.no_join, s.no_narrow_end, s.no_latency_sums, s.no_coop, s.no_piece_tree, s.convert_per_lane, s.top_per_sum,
                            s.piece_level_launches, s.sums_one_lane, (unsigned)s.piece_fuse_max, (unsigned)((unsigned long long)s.piece_fuse_max >> 32)};
    for (int i = 0; i < 11; i++) out[i] = v[i];
    return ok;
}
// plan: as emu_make_plan writes it; field: {own_records, g1_loose, pairs_built, pairs_default, words, bucket_bytes, coord_bytes};
// call: {fb_n, redo, may_defer, convert, flagged, stride, aligned16, top_cut}
// out: {steps, overflow, front, pieces, piece_cmax, piece_pending, small_sums, flag_with_sums, finalized, result, step capacity}, then
// per step {kernel, flag, rd0, rd1, wr0, wr1, block, gx, gy, lds, count, nthreads, fan, t, last, lgGB, lgG, m, sb, sp}
// returns the words written, 0 when the tail code is refused or |cap| words do not hold the route
extern "C" unsigned emu_make_route(const unsigned plan[21], const unsigned tun[13], const unsigned field[7], const unsigned* scalar_mod,
                                   unsigned scalar_words, const unsigned call[8], unsigned* out, unsigned cap)
{
    msm_plan p;
    p.n = plan[0]; p.wbits = plan[1]; p.nwins = plan[2]; p.NB = plan[3]; p.nbits = plan[4]; p.HB = plan[5]; p.LB = plan[6]; p.NA = plan[7];
    p.L = plan[8]; p.chunks_per_win = plan[9]; p.nslabs = plan[10]; p.slab_sz = plan[11]; p.F = plan[12]; p.K = plan[13]; p.K1 = plan[14];
    p.G = plan[15]; p.wpg = plan[16]; p.big = plan[17]; p.IB = plan[18]; p.SH = plan[19]; p.NG = plan[20];
    msm_tunables t;
    if (!tunables(tun, 0, t)) return 0;
    const msm_field f{field[0] != 0, field[1] != 0, field[2] != 0, field[3] != 0, field[4], field[5], field[6], scalar_mod, scalar_words};
    msm_call c;
    c.fb_n = call[0]; c.redo = call[1]; c.may_defer = call[2]; c.convert = call[3]; c.flagged = call[4]; c.stride = call[5];
    c.aligned16 = call[6]; c.top_cut = call[7];
    const msm_route r = make_route(p, t, f, c);
    if (cap < 11 + 20 * r.nsteps) return 0;
    const unsigned head[11] = {r.nsteps, r.overflow, r.front, r.pieces, r.piece_cmax, r.piece_pending, r.small_sums, r.flag_with_sums,
                               r.finalized, r.result, msm_route::CAP};
    unsigned* o = out;
    for (unsigned v : head) *o++ = v;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const msm_step& s = r.steps[i];
        const unsigned v[20] = {s.kernel, s.flag, s.rd[0], s.rd[1], s.wr[0], s.wr[1], s.block, s.gx, s.gy, s.lds, s.count, s.nthreads, s.fan,
                                s.t, s.last, s.lgGB, s.lgG, s.m, s.sb, s.sp};
        for (unsigned x : v) *o++ = x;
    }
    return (unsigned)(o - out);
}
