// HOST EMULATION TEST HARNESS (tests only; never linked into the product).
//
// accumulate_chunk (sppark_amd/csrc/msm/msm_kernels.hpp) on hand-built grouped lists, against a straightforward
// per-bucket sum.  The walk keeps its bucket offsets one boundary ahead and, where the field has a raw record form,
// its point gather one entry ahead and undecoded; what that could break is WHICH entries go into WHICH sum and where
// the sum is stored, and what is read beyond the arrays -- not the arithmetic.  So the model below does not walk: for
// every chunk it cuts the buckets that overlap [chunk L, chunk L + L) out of the offsets, adds each piece up with
// set() / madd() in list order, and places it by the contract at the head of accumulate_chunk (first piece -> record
// slot 0, last piece -> slot 1, pieces strictly inside -> buckets[key]).  Same operations in the same order, so
// every image must agree BIT FOR BIT, and every bucket and record that no piece owns must keep its fill pattern.
// The three input arrays end at an inaccessible page: a read past o[NB], past the last list entry or past the last
// point record ends the test with a fault instead of passing unnoticed.
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/msm/curve_select.hpp"
#include "../../sppark_amd/csrc/msm/msm_kernels.hpp"
#include <sys/mman.h>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace sppark_amd;

namespace {
// |bytes| bytes whose last one is the last accessible byte before a PROT_NONE page
struct guarded {
    unsigned char* map = nullptr; size_t len = 0; unsigned char* p = nullptr;
    guarded(const void* src, size_t bytes, size_t align)
    {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        const size_t body = (bytes + page - 1) / page * page + page;    // (a spare page: the start may move down for alignment)
        len = body + page;
        map = (unsigned char*)mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED) { map = nullptr; return; }
        p = map + body - bytes;
        p -= (size_t)p % align;                                         // (the callers' sizes are multiples of their alignment)
        memcpy(p, src, bytes);
        mprotect(map + body, page, PROT_NONE);
    }
    ~guarded() { if (map) munmap(map, len); }
};

typedef xyzz_dev<inst_fp> B;
typedef B::mem_t M;
constexpr u32 FILL = 0xa5a5a5a5u;

template<bool FLAGGED>
int check(const unsigned char* pts, unsigned stride, const u32* sorted, const u32* o, unsigned NB, unsigned L, unsigned* info)
{
    const unsigned total = o[NB];
    const unsigned chunks = (total + L - 1) / L + 1;                    // one chunk beyond the list: both keys NONE
    const unsigned w_base = 1;                                          // (the window's number in the whole MSM: keys and records)
    std::vector<M> got_b((size_t)2 * NB), exp_b((size_t)2 * NB), got_r((size_t)4 * chunks), exp_r((size_t)4 * chunks);
    std::vector<u32> got_k((size_t)4 * chunks, FILL), exp_k((size_t)4 * chunks, FILL);
    memset(got_b.data(), 0xa5, got_b.size() * sizeof(M)); memset(exp_b.data(), 0xa5, exp_b.size() * sizeof(M));
    memset(got_r.data(), 0xa5, got_r.size() * sizeof(M)); memset(exp_r.data(), 0xa5, exp_r.size() * sizeof(M));

    for (unsigned c = 0; c < chunks + 3; c++)                           // (work items past chunks_per_win return at once)
        accumulate_chunk<inst_fp, FLAGGED>(got_b.data(), got_k.data(), got_r.data(), pts, stride, sorted, o, total, NB, L, chunks, c, 0, w_base);

    unsigned pieces = 0, direct = 0;
    for (unsigned c = 0; c < chunks; c++) {
        const size_t rec0 = ((size_t)w_base * chunks + c) * 2;
        const unsigned lo = c * L, hi = total < lo + L ? total : lo + L;
        if (lo >= total) { exp_k[rec0] = KEY_NONE; exp_k[rec0 + 1] = KEY_NONE; continue; }
        struct piece { unsigned b, from, to; };
        std::vector<piece> ps;
        for (unsigned b = 0; b < NB; b++) {
            const unsigned from = o[b] > lo ? o[b] : lo, to = o[b + 1] < hi ? o[b + 1] : hi;
            if (from < to) ps.push_back({b, from, to});
        }
        for (size_t k = 0; k < ps.size(); k++) {
            B acc;
            for (unsigned q = ps[k].from; q < ps[k].to; q++) {
                const u32 e = sorted[q];
                const affine_dev<inst_fp> pt = load_affine<inst_fp, FLAGGED>(pts, e & 0x7fffffffu, stride);
                if (q == ps[k].from) acc.set(pt, e >> 31); else acc.madd(pt, e >> 31);
            }
            const u32 key = w_base * NB + ps[k].b;
            if (k == 0)                    { acc.store(&exp_r[rec0]); exp_k[rec0] = key; exp_k[rec0 + 1] = KEY_NONE; }
            else if (k + 1 == ps.size())   { acc.store(&exp_r[rec0 + 1]); exp_k[rec0 + 1] = key; }
            else                           { acc.store(&exp_b[key]); direct++; }
            pieces++;
        }
    }
    int bad = 0;
    for (size_t i = 0; i < got_k.size(); i++) if (got_k[i] != exp_k[i]) { if (!bad) fprintf(stderr, "emu_accumulate: key %zu: %08x, expected %08x\n", i, got_k[i], exp_k[i]); bad++; }
    for (size_t i = 0; i < got_r.size(); i++) if (memcmp(&got_r[i], &exp_r[i], sizeof(M))) { if (!bad) fprintf(stderr, "emu_accumulate: record %zu differs\n", i); bad++; }
    for (size_t i = 0; i < got_b.size(); i++) if (memcmp(&got_b[i], &exp_b[i], sizeof(M))) { if (!bad) fprintf(stderr, "emu_accumulate: bucket %zu differs\n", i); bad++; }
    if (info) { info[0] = pieces; info[1] = direct; info[2] = chunks; }
    return bad;
}
} // namespace

// |points|: npoints affine points in the wire format (plain, or flagged at |stride| bytes); |sorted|: o[NB] entries
// (point index, bit 31 = negate) grouped by bucket; |off|: the NB + 1 bucket offsets.  Returns the number of keys,
// records and buckets that differ from the model (-1: no memory); info = {pieces, buckets stored directly, chunks}.
extern "C" int emu_accumulate_check(const unsigned char* points, size_t stride, size_t npoints, int flagged,
                                    const unsigned* sorted, const unsigned* off, unsigned NB, unsigned L, unsigned* info)
{
    // the records the kernel gathers from: the field's own (converted as k_convert_points does) or the wire points
    std::vector<unsigned char> conv;
    const unsigned char* pts = points; size_t rec = stride;
    if constexpr (field_is_internal<inst_fp>::value) {
        rec = affine_loader<inst_fp>::STRIDE;
        conv.resize(npoints * rec);
        for (size_t i = 0; i < npoints; i++) {
            if (flagged) affine_loader<inst_fp>::template convert<true>(conv.data(), points, i, (unsigned)stride);
            else         affine_loader<inst_fp>::template convert<false>(conv.data(), points, i, (unsigned)stride);
        }
        pts = conv.data();
    }
    const unsigned total = off[NB];
    guarded gp(pts, npoints * rec, 16), gs(sorted, (size_t)total * 4, 4), go(off, ((size_t)NB + 1) * 4, 4);
    if (!gp.p || !gs.p || !go.p) return -1;
    return flagged ? check<true>(gp.p, (unsigned)stride, (const u32*)gs.p, (const u32*)go.p, NB, L, info)
                   : check<false>(gp.p, (unsigned)stride, (const u32*)gs.p, (const u32*)go.p, NB, L, info);
}
