// HOST TEST HARNESS (tests only): the per-work-item body of k_breakdown_short (sppark_amd/csrc/msm/msm_kernels.hpp
// breakdown_short_item -- load, mask, stage, recode) compiled for the host with -DSPPARK_HOST_EMULATION, checked by
// tests/test_msm_short_scalars.py over every declared bit length, every legal stride and every window count a plan can
// have.  With -DEMU_SHORT_SCALARS_MAIN the file is a stand-alone program that runs the whole sweep (the form a
// sanitizer build takes: every scalar array is an exact heap allocation, so a read past a scalar's stride is an error).
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/msm/curve_select.hpp"
#include "../../sppark_amd/csrc/msm/msm_kernels.hpp"
#include "../../sppark_amd/csrc/msm/msm_route.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sppark_amd;

namespace {
constexpr unsigned NBITS = curve_p::fr::NBITS;
constexpr unsigned MAX_WINDOW = 24;                     // make_plan's cap on the longest window

u64 splitmix(u64& x)
{
    u64 z = (x += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

// the digits of scalar |i| of |n| through the product's body, as the kernel instantiates it
void digits_of(u32* digits, const u32* scalars, size_t n, size_t i, unsigned bits, unsigned stride_words, unsigned nwins,
               unsigned w_begin, unsigned w_count)
{
    const unsigned nbits = bits + 1;
    u32 st[8 + 2];
    auto stage = [&](unsigned k) -> u32& { return st[k]; };
    switch (short_words_pow2((bits + 31) / 32)) {
    case 1:  breakdown_short_item<1>(digits, scalars, n, i, stage, nwins, nbits, stride_words, w_begin, w_count); break;
    case 2:  breakdown_short_item<2>(digits, scalars, n, i, stage, nwins, nbits, stride_words, w_begin, w_count); break;
    case 4:  breakdown_short_item<4>(digits, scalars, n, i, stage, nwins, nbits, stride_words, w_begin, w_count); break;
    default: breakdown_short_item<8>(digits, scalars, n, i, stage, nwins, nbits, stride_words, w_begin, w_count); break;
    }
}

// 320-bit accumulators: acc += d << off
void add_shifted(u64 (&acc)[5], u32 d, unsigned off)
{
    unsigned __int128 v = (unsigned __int128)d << (off & 63);
    unsigned k = off >> 6;
    u64 parts[2] = {(u64)v, (u64)(v >> 64)};
    unsigned c = 0;
    for (unsigned j = 0; k + j < 5; j++) {
        const u64 add = j < 2 ? parts[j] : 0;
        const u64 s0 = acc[k + j] + add, s1 = s0 + c;
        c = (s0 < add) || (s1 < s0);
        acc[k + j] = s1;
    }
}

struct failure { unsigned bits, stride, nwins, kind, what; };
}

// One cell: |bits| declared bits, |stride| bytes, |nwins| windows, scalar kind 0 = random, 1 = all ones (every bit of the
// slot set: the bits above |bits| must be masked), 2 = the single top bit 2^(bits-1) under garbage above bit |bits|.
// Checks: sum_w +-d_w 2^off_w == s mod 2^bits, |d_w| <= 2^(len_w - 1), every window group (w_begin, w_count) stores the
// digits of the whole run.  Returns 0, or 1 = sum, 2 = digit range, 3 = window group, 4 = neighbour touched.
extern "C" int emu_short_cell(unsigned bits, unsigned stride, unsigned nwins, unsigned kind, u64 seed)
{
    const unsigned nbits = bits + 1, sw = stride / 4;
    const size_t n = 3, i = 2;                          // the LAST scalar of an exact allocation: nothing may be read behind it
    u32* sc = (u32*)malloc(n * stride);
    u64 rng = seed ^ ((u64)bits << 40) ^ ((u64)stride << 32) ^ ((u64)nwins << 16) ^ kind;
    for (size_t k = 0; k < n * sw; k++) sc[k] = kind == 1 ? ~0u : (u32)splitmix(rng);
    u32* mine = sc + i * sw;
    if (kind == 2) {
        for (unsigned k = 0; k < (bits + 31) / 32; k++) mine[k] = 0;        // (words above those of |bits| keep their garbage)
        mine[(bits - 1) >> 5] = 1u << ((bits - 1) & 31);
        if (bits & 31) mine[(bits - 1) >> 5] |= ~0u << (bits & 31);         // garbage from bit |bits| up
    }
    // s mod 2^bits
    u64 want[5] = {0, 0, 0, 0, 0};
    for (unsigned k = 0; k < (bits + 31) / 32; k++) {
        u32 w = mine[k];
        if (k == (bits - 1) / 32 && (bits & 31)) w &= (1u << (bits & 31)) - 1;
        want[k >> 1] |= (u64)w << (32 * (k & 1));
    }
    std::vector<u32> full((size_t)nwins * n, 0xdeadbeefu);
    digits_of(full.data(), sc, n, i, bits, sw, nwins, 0, ~0u);
    int rc = 0;
    u64 pos[5] = {0, 0, 0, 0, 0}, neg[5] = {0, 0, 0, 0, 0};
    for (unsigned w = 0, off = 0; w < nwins; w++) {
        const unsigned len = window_len(w, nwins, nbits);
        const u32 d = full[(size_t)w * n + i], mag = d & 0x7fffffffu;
        if (mag > (1u << (len - 1)) || (d >> 31 && mag == 0)) rc = rc ? rc : 2;
        add_shifted(d >> 31 ? neg : pos, mag, off);
        off += len;
        for (size_t j = 0; j < n; j++) if (j != i && full[(size_t)w * n + j] != 0xdeadbeefu) rc = rc ? rc : 4;
    }
    {   // pos - neg == want
        unsigned bw = 0;
        for (unsigned k = 0; k < 5; k++) {
            const u64 a = pos[k], b = neg[k], d0 = a - b, d1 = d0 - bw;
            bw = (a < b) || (d0 < bw);
            if (d1 != want[k]) rc = rc ? rc : 1;
        }
        if (bw) rc = rc ? rc : 1;
    }
    // window groups: every split into groups of g windows, g = 1 .. nwins
    for (unsigned g = 1; g <= nwins && !rc; g++)
        for (unsigned w0 = 0; w0 < nwins && !rc; w0 += g) {
            const unsigned wn = nwins - w0 < g ? nwins - w0 : g;
            std::vector<u32> part((size_t)wn * n, 0xdeadbeefu);
            digits_of(part.data(), sc, n, i, bits, sw, nwins, w0, g);
            for (unsigned w = 0; w < wn; w++) if (part[(size_t)w * n + i] != full[(size_t)(w0 + w) * n + i]) rc = 3;
        }
    free(sc);
    return rc;
}

// the whole sweep: bits 1 .. NBITS - 2, every legal stride, every window count 1 .. ceil((bits + 1) / 2) whose longest window
// is within the plan's cap, the three scalar kinds.  Returns the number of cells run; *failed = how many failed,
// first[5] = {bits, stride, nwins, kind, code} of the first failure.
extern "C" unsigned long emu_short_sweep(u64 seed, unsigned* failed, unsigned first[5])
{
    unsigned long cells = 0;
    *failed = 0;
    for (unsigned bits = 1; bits <= NBITS - 2; bits++)
        for (unsigned stride = 4 * ((bits + 31) / 32); stride <= 32; stride += 4)
            for (unsigned nwins = 1; nwins <= (bits + 2) / 2; nwins++) {
                if ((bits + 1 + nwins - 1) / nwins > MAX_WINDOW) continue;
                for (unsigned kind = 0; kind < 3; kind++) {
                    const int rc = emu_short_cell(bits, stride, nwins, kind, seed);
                    cells++;
                    if (rc && (*failed)++ == 0) { first[0] = bits; first[1] = stride; first[2] = nwins; first[3] = kind; first[4] = (unsigned)rc; }
                }
            }
    return cells;
}

extern "C" unsigned emu_short_nbits() { return NBITS; }

// ---- the plan and the route of a short call (msm_route.hpp with msm_call::short_bits), in the flat form of
// tests/emu/emu_plan.cpp's emu_make_plan_tuned / emu_make_route; short_bits == 0: the full-width call ----
// tun: {wbits, L, F, K, nslabs, LB, groups, K1, records, top, tail code, g2 path, long_runs}; field: {own_records, g1_loose,
// pairs_built, pairs_default, words, bucket_bytes, coord_bytes}; call: {fb_n, redo, may_defer, convert, flagged, stride, aligned16, top_cut}
extern "C" unsigned emu_short_route(size_t npoints, unsigned plan_bits, const unsigned tun[13], size_t resident_lanes, const unsigned field[7],
                                    const unsigned call[8], unsigned short_bits, unsigned plan_out[21], unsigned* out, unsigned cap)
{
    msm_tunables t;
    t.wbits = tun[0]; t.L = tun[1]; t.F = tun[2]; t.K = tun[3]; t.nslabs = tun[4]; t.LB = tun[5]; t.groups = tun[6]; t.K1 = tun[7];
    t.records = tun[8]; t.top = tun[9]; t.g2_coop = tun[11]; t.long_runs = tun[12]; t.resident_lanes = resident_lanes;
    if (!decode_tail_code(tun[10], t.sw)) return 0;
    const msm_plan p = make_plan(npoints, plan_bits, t);
    const unsigned pv[21] = {p.n, p.wbits, p.nwins, p.NB, p.nbits, p.HB, p.LB, p.NA, p.L, p.chunks_per_win, p.nslabs, p.slab_sz,
                             p.F, p.K, p.K1, p.G, p.wpg, p.big, p.IB, p.SH, p.NG};
    for (int i = 0; i < 21; i++) plan_out[i] = pv[i];
    const msm_field f{field[0] != 0, field[1] != 0, field[2] != 0, field[3] != 0, field[4], field[5], field[6], curve_p::fr::MOD, (unsigned)curve_p::fr::N};
    msm_call c;
    c.fb_n = call[0]; c.redo = call[1]; c.may_defer = call[2]; c.convert = call[3]; c.flagged = call[4]; c.stride = call[5];
    c.aligned16 = call[6]; c.top_cut = call[7]; c.short_bits = short_bits;
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

// The fullest bucket of a UNIFORM short input in PIECES: n scalars with |bits| random bits through the product's body,
// the window's grouped list cut into runs of L entries as k_accumulate cuts it; a bucket's pieces are the runs it touches.
// (What the piece tree's size -- piece_tree_cmax with the short bound -- must cover for the tail not to run twice.)
extern "C" unsigned emu_short_max_pieces(unsigned n, unsigned bits, unsigned nwins, unsigned L, u64 seed)
{
    const unsigned sw = (bits + 31) / 32, nbits = bits + 1;
    std::vector<u32> sc((size_t)n * sw);
    u64 rng = seed;
    for (auto& w : sc) w = (u32)splitmix(rng);
    std::vector<u32> digits((size_t)nwins * n);
    for (unsigned i = 0; i < n; i++) digits_of(digits.data(), sc.data(), n, i, bits, sw, nwins, 0, ~0u);
    unsigned worst = 0;
    for (unsigned w = 0; w < nwins; w++) {
        const unsigned NBk = 1u << window_len(0, nwins, nbits);            // (more than enough: the longest window's range)
        std::vector<u32> cnt(NBk + 1, 0);
        for (unsigned i = 0; i < n; i++) { const u32 m = digits[(size_t)w * n + i] & 0x7fffffffu; if (m) cnt[m]++; }
        size_t start = 0;
        for (unsigned b = 1; b <= NBk; b++) {
            if (!cnt[b]) continue;
            const size_t end = start + cnt[b];
            const unsigned pieces = (unsigned)((end - 1) / L - start / L + 1);
            if (pieces > worst) worst = pieces;
            start = end;
        }
    }
    return worst;
}

#ifdef EMU_SHORT_SCALARS_MAIN
int main()
{
    unsigned failed = 0, first[5] = {0, 0, 0, 0, 0};
    const unsigned long cells = emu_short_sweep(0x5eedULL, &failed, first);
    printf("k_breakdown_short body: %lu cells, %u failed", cells, failed);
    if (failed) printf(" (first: bits %u stride %u windows %u kind %u code %u)", first[0], first[1], first[2], first[3], first[4]);
    printf("\n");
    return failed ? 1 : 0;
}
#endif
