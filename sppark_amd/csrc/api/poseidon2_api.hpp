// C entry points of Poseidon2 over the library's field fr_t (include/sppark_amd_poseidon2.h): the permutation over a vector
// of states and the commitment to a matrix.  BabyBear and Goldilocks libraries only.  The launches are those of
// poseidon2/poseidon2_route.hpp: the drivers below run what the route says.  The matrix arguments, their checks and the
// tree are those of merkle_api.hpp.
// Expects fr_t in scope.
#pragma once
#include "merkle_api.hpp"
#include "../poseidon2/poseidon2_kernels.hpp"

namespace {
constexpr unsigned P2_T = p2_shape<fr_t>::T;
typedef p2_digest<fr_t> p2_dg;
typedef p2_state<fr_t> p2_st;
static_assert(sizeof(p2_dg) == sizeof(mk_digest) && sizeof(p2_st) == 64, "a digest is 32 bytes, a state 64");

// the constants and the round numbers; the bytes of the constants buffer
size_t poseidon2_consts_of(const void* consts, uint32_t rounds_f, uint32_t rounds_p, const std::string& who)
{
    if (consts == nullptr) reject(who + ": NULL consts");
    if (rounds_f < 2 || rounds_f > P2_MAX_RF || (rounds_f & 1)) reject(who + ": rounds_f is not an even number 2 .. " + std::to_string(P2_MAX_RF));
    if (rounds_p > P2_MAX_RP) reject(who + ": rounds_p above " + std::to_string(P2_MAX_RP));
    if ((uintptr_t)consts % sizeof(fr_t)) reject(who + ": misaligned consts");
    return p2_const_count(P2_T, rounds_f, rounds_p) * sizeof(fr_t);
}

void poseidon2_permute_any(size_t device_id, void* out, const void* in, size_t count, const void* consts, uint32_t rounds_f,
                           uint32_t rounds_p, hipStream_t s)
{
    const std::string who("sppark_poseidon2_permute");
    if (out == nullptr || in == nullptr) reject(who + ": NULL buffer");
    const size_t bytes = checked_mul(count, sizeof(p2_st), who.c_str(), ": count * 64 overflows size_t");
    const size_t cbytes = poseidon2_consts_of(consts, rounds_f, rounds_p, who);
    if (((uintptr_t)out | (uintptr_t)in) & 15) reject(who + ": misaligned out or in (16 bytes)");
    same_or_disjoint(out, in, bytes, "sppark_poseidon2_permute: out and in overlap in part: invalid argument");
    if (bytes && ranges_meet(out, bytes, consts, cbytes)) reject(who + ": consts may not overlap out");
    if (count == 0) return;
    const gpu_info& gpu = select_gpu((int)device_id);

    p2_call c;
    c.op = P2_OP_PERMUTE; c.elem_bytes = sizeof(fr_t); c.rounds_f = rounds_f; c.rounds_p = rounds_p; c.count = count;
    c.cus = (unsigned)gpu.prop.multiProcessorCount;
    const p2_route route = make_poseidon2_route(c);
    if (route.invalid) reject(who + ": no route");

    call_scope sc(s);
    const fr_t* d_c = sc.in<fr_t>(consts, cbytes / sizeof(fr_t));
    const p2_st* d_in = sc.in<p2_st>(in, count);
    p2_st* d_out = sc.out<p2_st>(out, count);                                // (out == in on the host: the same device buffer)
    for (unsigned i = 0; i < route.nsteps; i++) {
        const p2_step& st = route.steps[i];
        hipLaunchKernelGGL((k_p2_permute<fr_t>), dim3(st.grid), dim3(st.block), 0, s, d_out, d_in, st.items, d_c, rounds_f, rounds_p);
        HIP_OK(hipGetLastError());
    }
    sc.finish();
}

void poseidon2_commit_any(size_t device_id, void* tree, void* root, const void* in, uint32_t lg_n, size_t width, size_t col_stride,
                          size_t leaf_stride, const void* consts, uint32_t rounds_f, uint32_t rounds_p, hipStream_t s)
{
    const std::string who("sppark_poseidon2_commit");
    if (tree == nullptr) reject(who + ": NULL tree");
    merkle_matrix m = merkle_matrix_of(in, lg_n, width, col_stride, leaf_stride, who);
    const size_t cbytes = poseidon2_consts_of(consts, rounds_f, rounds_p, who);
    if ((uintptr_t)tree & 15) reject(who + ": misaligned tree (16 bytes)");
    const size_t tree_bytes = (((size_t)2 << lg_n) - 1) * sizeof(p2_dg);
    if (ranges_meet(tree, tree_bytes, in, m.span_bytes)) reject(who + ": tree may not overlap in");
    if (root != nullptr && ranges_meet(root, sizeof(p2_dg), in, m.span_bytes)) reject(who + ": root may not overlap in");
    if (root != nullptr && ranges_meet(root, sizeof(p2_dg), tree, tree_bytes))
        reject(who + ": root may not lie inside tree (the root is the tree's last 32 bytes)");
    if (ranges_meet(tree, tree_bytes, consts, cbytes)) reject(who + ": consts may not overlap tree");
    if (root != nullptr && ranges_meet(root, sizeof(p2_dg), consts, cbytes)) reject(who + ": consts may not overlap root");
    const gpu_info& gpu = select_gpu((int)device_id);

    p2_call c;
    c.op = P2_OP_COMMIT; c.elem_bytes = sizeof(fr_t); c.rounds_f = rounds_f; c.rounds_p = rounds_p;
    c.lg_n = lg_n; c.width = width; c.layout = m.layout; c.cus = (unsigned)gpu.prop.multiProcessorCount;
    const p2_route route = make_poseidon2_route(c);
    if (route.invalid) reject(who + ": no route");

    const bool root_dev = root != nullptr && is_device_pointer(root), root_aligned = ((uintptr_t)root & 15) == 0;
    call_scope sc(s);
    const fr_t* d_c = sc.in<fr_t>(consts, cbytes / sizeof(fr_t));
    const fr_t* d_in = (const fr_t*)merkle_matrix_in(sc, in, m);
    p2_dg* d_tree = (p2_dg*)sc.out<char>(tree, tree_bytes);
    p2_dg* d_root = root_dev && root_aligned ? (p2_dg*)root : nullptr;       // (the kernel writes an aligned device root itself)
    for (unsigned i = 0; i < route.nsteps; i++) {
        const p2_step& st = route.steps[i];
        const dim3 grid(st.grid), block(st.block);
        if (st.kernel == P2K_LEAVES) {
            if (m.layout == MERKLE_COLUMNS)
                hipLaunchKernelGGL((k_p2_leaves<fr_t, true>), grid, block, 0, s, d_tree, d_in, m.n, m.width, m.col_stride, m.leaf_stride, d_c, rounds_f, rounds_p);
            else
                hipLaunchKernelGGL((k_p2_leaves<fr_t, false>), grid, block, 0, s, d_tree, d_in, m.n, m.width, m.col_stride, m.leaf_stride, d_c, rounds_f, rounds_p);
        } else if (st.kernel == P2K_NODES) {
            hipLaunchKernelGGL((k_p2_nodes<fr_t, P2_S>), grid, block, 0, s, d_tree, lg_n, st.first, st.items, d_c, rounds_f, rounds_p);
        } else if (st.kernel == P2K_TOP) {
            hipLaunchKernelGGL((k_p2_top<fr_t>), grid, block, 0, s, d_tree, d_root, lg_n, st.first, d_c, rounds_f, rounds_p);
        } else {
            reject(who + ": a step that is not a commitment's");
        }
        HIP_OK(hipGetLastError());
    }
    const char* top = (const char*)d_tree + tree_bytes - sizeof(p2_dg);
    if (root != nullptr && !root_dev) sc.copy_out(root, top, sizeof(p2_dg));
    else if (root != nullptr && d_root == nullptr) HIP_OK(hipMemcpyAsync(root, top, sizeof(p2_dg), hipMemcpyDefault, s));
    sc.finish();                        // (everything on the device and a stream: only enqueued)
}
}

SPPARK_FFI RustError sppark_poseidon2_permute(size_t device_id, void* out, const void* in, size_t count, const void* consts,
                                              uint32_t rounds_f, uint32_t rounds_p, void* stream)
{   return guarded([&] { poseidon2_permute_any(device_id, out, in, count, consts, rounds_f, rounds_p, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_poseidon2_commit(size_t device_id, void* tree, void* root, const void* in, uint32_t lg_n, size_t width,
                                             size_t col_stride, size_t leaf_stride, const void* consts, uint32_t rounds_f, uint32_t rounds_p,
                                             void* stream)
{
    return guarded([&] { poseidon2_commit_any(device_id, tree, root, in, lg_n, width, col_stride, leaf_stride, consts, rounds_f, rounds_p,
                                              (hipStream_t)stream); });
}
