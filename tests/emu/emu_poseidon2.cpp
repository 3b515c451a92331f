// HOST EMULATION TEST HARNESS for the Poseidon2 kernels (tests only; see emu_merkle.cpp).
// Runs the bodies of sppark_amd/csrc/poseidon2/poseidon2_kernels.hpp for every (work-group, lane) the GPU grid would cover,
// over the steps of the driver's own route (poseidon2_route.hpp make_poseidon2_route): no decision is made here.  The top
// kernel's barrier between two levels is the end of a loop over the lanes here, its two LDS buffers two arrays.  The field
// classes are the device's own (ff/small_fields_dev.hpp, their plain C++ paths): one shared library, both fields, chosen by
// the element's size.  With -DEMU_POSEIDON2_MAIN the file is a stand-alone program that checks itself across layouts and
// against the definition's properties (for a sanitizer run).
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/poseidon2/poseidon2_kernels.hpp"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace sppark_amd;

// ---- the route as integers (tests/test_poseidon2_route.py) ----
// call: {op, elem_bytes, rounds_f, rounds_p, count, lg_n, width, layout, cus}
// out: {nsteps, invalid}, then per step {kernel, grid, block, first, lo, hi, fused, items}
static p2_call call_of(const uint64_t call[9])
{
    p2_call c;
    c.op = (int)call[0]; c.elem_bytes = (size_t)call[1]; c.rounds_f = (unsigned)call[2]; c.rounds_p = (unsigned)call[3];
    c.count = (size_t)call[4]; c.lg_n = (unsigned)call[5]; c.width = (size_t)call[6]; c.layout = (int)call[7]; c.cus = (unsigned)call[8];
    return c;
}
extern "C" unsigned emu_p2_route(const uint64_t call[9], uint64_t* out, unsigned cap)
{
    const p2_route r = make_poseidon2_route(call_of(call));
    if (cap < 2 + 8 * r.nsteps) return 0;
    uint64_t* o = out;
    *o++ = r.nsteps; *o++ = r.invalid;
    for (unsigned i = 0; i < r.nsteps; i++) {
        const p2_step& s = r.steps[i];
        const uint64_t v[8] = {s.kernel, s.grid, s.block, s.first, s.lo, s.hi, s.fused, s.items};
        for (uint64_t x : v) *o++ = x;
    }
    return (unsigned)(o - out);
}
extern "C" unsigned emu_p2_top() { return P2_TOP; }
extern "C" unsigned emu_p2_fused() { return P2_S; }
extern "C" unsigned emu_p2_wg_per_cu() { return P2_WG_PER_CU; }
extern "C" unsigned emu_p2_width(unsigned elem_bytes) { return p2_width_of(elem_bytes); }

template<class F>
static int permute_run(void* out, const void* in, size_t count, const void* consts, unsigned rf, unsigned rp, unsigned cus)
{
    p2_call c;
    c.op = P2_OP_PERMUTE; c.elem_bytes = sizeof(F); c.rounds_f = rf; c.rounds_p = rp; c.count = count; c.cus = cus;
    const p2_route rt = make_poseidon2_route(c);
    if (rt.invalid || rt.nsteps != 1 || rt.steps[0].kernel != P2K_PERMUTE || rt.steps[0].block != P2_NT) return -1;
    const p2_step& s = rt.steps[0];
    for (unsigned b = 0; b < s.grid; b++)
        for (unsigned t = 0; t < s.block; t++)
            p2_permute_lane<F>((p2_state<F>*)out, (const p2_state<F>*)in, s.items, (const F*)consts, rf, rp, b, s.grid, t);
    return 0;
}

template<class F>
static void top_run(p2_digest<F>* tree, p2_digest<F>* root, unsigned lg_n, unsigned first, const F* c, unsigned rf, unsigned rp)
{
    std::vector<p2_digest<F>> even(P2_TOP / 2), odd(P2_TOP / 4);
    const p2_digest<F>* src = tree + merkle_layer_offset(lg_n, first);
    for (unsigned l = first; l < lg_n; l++) {
        p2_digest<F>* keep = ((l - first) & 1) ? odd.data() : even.data();
        for (unsigned t = 0; t < P2_NT; t++)
            p2_top_level<F>(tree + merkle_layer_offset(lg_n, l + 1), keep, src, (size_t)1 << (lg_n - l - 1), c, rf, rp, t);
        src = keep;
    }
    if (root != nullptr) *root = *src;
}

template<class F>
static int commit_run(void* tree_, void* root_, const void* in_, unsigned lg_n, size_t width, size_t cs, size_t ls, int layout,
                      const void* consts, unsigned rf, unsigned rp, unsigned cus)
{
    p2_digest<F>* tree = (p2_digest<F>*)tree_;
    p2_digest<F>* root = (p2_digest<F>*)root_;
    const F* in = (const F*)in_;
    const F* k = (const F*)consts;
    p2_call c;
    c.op = P2_OP_COMMIT; c.elem_bytes = sizeof(F); c.rounds_f = rf; c.rounds_p = rp; c.lg_n = lg_n; c.width = width; c.layout = layout; c.cus = cus;
    const p2_route rt = make_poseidon2_route(c);
    if (rt.invalid || rt.nsteps < 2) return -1;
    const size_t n = (size_t)1 << lg_n;
    for (unsigned i = 0; i < rt.nsteps; i++) {
        const p2_step& s = rt.steps[i];
        if (s.block != P2_NT) return -1;
        if (s.kernel == P2K_LEAVES) {
            for (unsigned b = 0; b < s.grid; b++)
                for (unsigned t = 0; t < s.block; t++) {
                    if (layout == MERKLE_COLUMNS) p2_leaf_lane<F, true>(tree, in, n, width, cs, ls, k, rf, rp, b, s.grid, t);
                    else                          p2_leaf_lane<F, false>(tree, in, n, width, cs, ls, k, rf, rp, b, s.grid, t);
                }
        } else if (s.kernel == P2K_NODES) {
            if (s.fused != P2_S || s.lo != s.first + 1) return -1;
            for (unsigned b = 0; b < s.grid; b++)
                for (unsigned t = 0; t < s.block; t++) p2_nodes_lane<F, P2_S>(tree, lg_n, s.first, s.items, k, rf, rp, b, s.grid, t);
        } else if (s.kernel == P2K_TOP) {
            if (s.grid != 1 || s.items > P2_TOP) return -1;
            top_run<F>(tree, root, lg_n, s.first, k, rf, rp);
        } else return -1;
    }
    return 0;
}

// out, in: 16-byte aligned, count * 64 bytes; consts: aligned to the element
extern "C" int emu_p2_permute(void* out, const void* in, size_t count, unsigned elem_bytes, const void* consts, unsigned rf, unsigned rp,
                              unsigned cus)
{
    if (((uintptr_t)out | (uintptr_t)in) & 15 || (uintptr_t)consts % elem_bytes) return -3;
    if (elem_bytes == 4) return permute_run<bb31_dev>(out, in, count, consts, rf, rp, cus);
    if (elem_bytes == 8) return permute_run<gl64_dev>(out, in, count, consts, rf, rp, cus);
    return -5;
}

// tree: 16-byte aligned, (2^(lg_n+1) - 1) * 32 bytes; root: 16-byte aligned or NULL; in, consts: aligned to the element
extern "C" int emu_p2_commit(void* tree, void* root, const void* in, unsigned elem_bytes, unsigned lg_n, size_t width, size_t col_stride,
                             size_t leaf_stride, const void* consts, unsigned rf, unsigned rp, unsigned cus)
{
    const int layout = leaf_stride == 1 && col_stride >= ((size_t)1 << lg_n) ? MERKLE_COLUMNS : MERKLE_ROWS;
    if (layout == MERKLE_ROWS && !(col_stride == 1 && leaf_stride >= width)) return -2;
    if (((uintptr_t)tree | (uintptr_t)root) & 15 || (uintptr_t)in % elem_bytes || (uintptr_t)consts % elem_bytes) return -3;
    if (elem_bytes == 4) return commit_run<bb31_dev>(tree, root, in, lg_n, width, col_stride, leaf_stride, layout, consts, rf, rp, cus);
    if (elem_bytes == 8) return commit_run<gl64_dev>(tree, root, in, lg_n, width, col_stride, leaf_stride, layout, consts, rf, rp, cus);
    return -5;
}

#ifdef EMU_POSEIDON2_MAIN
// Stand-alone self-check, both fields, constants from a xorshift stream reduced below p: the columns and the rows tree of
// the same leaves (padded strides) are the same bytes; every node is the permutation of its two children, truncated; a leaf of
// RATE elements is the permutation of (leaf || 0); the root copy equals the tree's last digest; lg_n 0 .. 14.
static uint64_t g_seed = 0x9e3779b97f4a7c15ULL;
static uint64_t next64() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return g_seed; }
struct alignas(16) q16 { unsigned char b[16]; };
typedef std::vector<q16> buffer;
static buffer bytes_of(size_t n) { return buffer((n + 15) / 16 + 1); }

template<class F> static F rnd() { return F::from_raw((typename F::word_t)(next64() % F::MOD)); }

template<class F> static int self_check()
{
    constexpr unsigned T = p2_shape<F>::T, RATE = T / 2, EB = sizeof(F);
    const unsigned cus = 2;
    int bad = 0;
    const unsigned rounds[3][2] = {{2, 0}, {8, 1}, {8, T == 16 ? 13u : 22u}};
    for (auto& rr : rounds) {
        const unsigned rf = rr[0], rp = rr[1];
        std::vector<F> k(p2_const_count(T, rf, rp));
        for (F& x : k) x = rnd<F>();
        const size_t widths[] = {1, RATE - 1, RATE, RATE + 1, 2 * RATE, 2 * RATE + 1};
        for (unsigned lg = 0; lg <= 14; lg += (lg >= 11 ? 3 : 1))
            for (size_t width : widths) {
                if (lg > 8 && width != RATE + 1) continue;
                const size_t n = (size_t)1 << lg, cs = n + 3, ls = width + 2, tb = (2 * n - 1) * 32;
                buffer cols = bytes_of(width * cs * EB), rows = bytes_of(n * ls * EB);
                F* pc = (F*)cols.data();
                F* pr = (F*)rows.data();
                for (size_t i = 0; i < width * cs; i++) pc[i] = rnd<F>();
                for (size_t i = 0; i < n * ls; i++) pr[i] = rnd<F>();
                for (size_t i = 0; i < n; i++)
                    for (size_t j = 0; j < width; j++) pr[i * ls + j] = pc[j * cs + i];
                buffer t1 = bytes_of(tb), t2 = bytes_of(tb), root = bytes_of(32);
                if (emu_p2_commit(t1.data(), root.data(), cols.data(), EB, lg, width, cs, 1, k.data(), rf, rp, cus)) bad++;
                if (emu_p2_commit(t2.data(), nullptr, rows.data(), EB, lg, width, 1, ls, k.data(), rf, rp, cus)) bad++;
                if (memcmp(t1.data(), t2.data(), tb)) { bad++; printf("EB %u lg %u width %zu: trees differ\n", EB, lg, width); }
                if (memcmp(root.data(), (char*)t1.data() + tb - 32, 32)) bad++;
                const p2_digest<F>* tree = (const p2_digest<F>*)t1.data();
                for (unsigned l = 0; l < lg; l++)                                          // nodes through the permute entry
                    for (size_t i = 0; i < ((size_t)1 << (lg - l - 1)); i += (lg > 8 ? 37 : 1)) {
                        buffer st = bytes_of(64), o = bytes_of(64);
                        memcpy(st.data(), &tree[merkle_layer_offset(lg, l) + 2 * i], 64);
                        if (emu_p2_permute(o.data(), st.data(), 1, EB, k.data(), rf, rp, cus)) bad++;
                        if (memcmp(o.data(), &tree[merkle_layer_offset(lg, l + 1) + i], 32)) { bad++; printf("lg %u layer %u node %zu differs\n", lg, l + 1, i); }
                    }
                if (width == RATE) {
                    buffer st = bytes_of(64), o = bytes_of(64);
                    memset(st.data(), 0, 64);
                    for (size_t j = 0; j < width; j++) ((F*)st.data())[j] = pc[j * cs];
                    if (emu_p2_permute(o.data(), st.data(), 1, EB, k.data(), rf, rp, cus)) bad++;
                    if (memcmp(o.data(), &tree[0], 32)) { bad++; printf("lg %u: leaf 0 differs\n", lg); }
                }
            }
        // in place equals out of place
        const size_t count = 600;
        buffer a = bytes_of(count * 64), b = bytes_of(count * 64);
        for (size_t i = 0; i < count * T; i++) ((F*)a.data())[i] = rnd<F>();
        if (emu_p2_permute(b.data(), a.data(), count, EB, k.data(), rf, rp, cus)) bad++;
        if (emu_p2_permute(a.data(), a.data(), count, EB, k.data(), rf, rp, cus)) bad++;
        if (memcmp(a.data(), b.data(), count * 64)) { bad++; printf("in place differs\n"); }
    }
    return bad;
}

int main()
{
    const int bad = self_check<bb31_dev>() + self_check<gl64_dev>();
    printf("emu_poseidon2 self-check, both fields, lg_n 0 .. 14: %s (%d mismatches)\n", bad ? "FAILED" : "ok", bad);
    return bad ? 1 : 0;
}
#endif
