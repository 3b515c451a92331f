// C entry points of the Merkle commitments over matrices of the library's field fr_t (include/sppark_amd_merkle.h).
// The launches are those of merkle/merkle_route.hpp: the driver below runs what the route says.  The kernels see the
// elements as sizeof(fr_t) / 4 opaque words.
// Expects fr_t in scope.
#pragma once
#include "call.hpp"
#include "../merkle/merkle_kernels.hpp"
#include <vector>

namespace {
constexpr unsigned MERKLE_EW = sizeof(fr_t) / 4;
static_assert(sizeof(fr_t) == 4 || sizeof(fr_t) == 8 || sizeof(fr_t) == 16 || sizeof(fr_t) == 32, "elements of 1, 2, 4 or 8 words");
constexpr const char* MERKLE_OVERFLOW = ": a size overflows size_t";

struct merkle_matrix { size_t n, width, col_stride, leaf_stride, span_bytes; int layout; };

// the matrix arguments of commit and gather: the layout and the bytes from the first element to the end of the last
merkle_matrix merkle_matrix_of(const void* in, uint32_t lg_n, size_t width, size_t col_stride, size_t leaf_stride, const std::string& who)
{
    if (in == nullptr) reject(who + ": NULL in");
    if (lg_n > MERKLE_MAX_LG) reject(who + ": lg_n above " + std::to_string(MERKLE_MAX_LG));
    if (width == 0) reject(who + ": width == 0");
    if (width > (size_t)0xffffffffu / sizeof(fr_t)) reject(who + ": width * sizeof(element) reaches 2^32");
    merkle_matrix m;
    m.n = (size_t)1 << lg_n; m.width = width; m.col_stride = col_stride; m.leaf_stride = leaf_stride;
    if (leaf_stride == 1 && col_stride >= m.n) m.layout = MERKLE_COLUMNS;
    else if (col_stride == 1 && leaf_stride >= width) m.layout = MERKLE_ROWS;
    else reject(who + ": strides are neither columns (leaf_stride == 1, col_stride >= n) nor rows (col_stride == 1, leaf_stride >= width)");
    const char* w = who.c_str();
    const size_t last = checked_add(checked_mul(width - 1, col_stride, w, MERKLE_OVERFLOW), checked_mul(m.n - 1, leaf_stride, w, MERKLE_OVERFLOW), w, MERKLE_OVERFLOW);
    m.span_bytes = checked_mul(checked_add(last, 1, w, MERKLE_OVERFLOW), sizeof(fr_t), w, MERKLE_OVERFLOW);
    if ((uintptr_t)in % (sizeof(fr_t) < 16 ? sizeof(fr_t) : 16)) reject(who + ": misaligned in");
    return m;
}

void merkle_check_indices(const uint64_t* indices, size_t nidx, uint32_t lg_n, const std::string& who)
{
    if (nidx && indices == nullptr) reject(who + ": NULL indices with nidx > 0");
    for (size_t q = 0; q < nidx; q++)
        if (indices[q] >> lg_n) reject(who + ": index " + std::to_string(q) + " is not below n");
}

// the matrix on the device: a device matrix as it is; of a host matrix a packed copy (only the elements are read, never the
// gaps of a stride), with |m|'s stride set to match
const void* merkle_matrix_in(call_scope& sc, const void* in, merkle_matrix& m)
{
    const bool cols = m.layout == MERKLE_COLUMNS;
    const size_t line = cols ? m.n : m.width, lines = cols ? m.width : m.n;
    const void* d = sc.in_lines<fr_t>(in, line, lines, cols ? m.col_stride : m.leaf_stride);
    if (d != in) { if (cols) m.col_stride = m.n; else m.leaf_stride = m.width; }
    return d;
}

template<int HASH>
void merkle_run(const merkle_route& route, mk_digest* tree, mk_digest* root, const void* in, const merkle_matrix& m, uint32_t lg_n, hipStream_t s)
{
    for (unsigned i = 0; i < route.nsteps; i++) {
        const merkle_step& st = route.steps[i];
        const dim3 grid(st.grid), block(st.block);
        if (st.kernel == MKK_LEAVES) {
            if (m.layout == MERKLE_COLUMNS)
                hipLaunchKernelGGL((k_merkle_leaves<MERKLE_EW, HASH, true>), grid, block, 0, s, tree, in, m.n, m.width, m.col_stride, m.leaf_stride);
            else
                hipLaunchKernelGGL((k_merkle_leaves<MERKLE_EW, HASH, false>), grid, block, 0, s, tree, in, m.n, m.width, m.col_stride, m.leaf_stride);
        } else if (st.kernel == MKK_NODES) {
            hipLaunchKernelGGL((k_merkle_nodes<HASH, MERKLE_S>), grid, block, 0, s, tree, lg_n, st.first, st.items);
        } else {
            hipLaunchKernelGGL((k_merkle_top<HASH>), grid, block, 0, s, tree, root, lg_n, st.first);
        }
        HIP_OK(hipGetLastError());
    }
}

void merkle_commit_any(size_t device_id, void* tree, void* root, const void* in, uint32_t lg_n, size_t width, size_t col_stride,
                       size_t leaf_stride, int hash, hipStream_t s)
{
    const std::string who("sppark_merkle_commit");
    if (tree == nullptr) reject(who + ": NULL tree");
    merkle_matrix m = merkle_matrix_of(in, lg_n, width, col_stride, leaf_stride, who);
    if (hash != MERKLE_BLAKE2S && hash != MERKLE_SHA256) reject(who + ": unknown hash");
    if ((uintptr_t)tree & 15) reject(who + ": misaligned tree (16 bytes)");
    const size_t tree_bytes = (((size_t)2 << lg_n) - 1) * sizeof(mk_digest);
    if (ranges_meet(tree, tree_bytes, in, m.span_bytes)) reject(who + ": tree may not overlap in");
    if (root != nullptr && ranges_meet(root, sizeof(mk_digest), in, m.span_bytes)) reject(who + ": root may not overlap in");
    if (root != nullptr && ranges_meet(root, sizeof(mk_digest), tree, tree_bytes))
        reject(who + ": root may not lie inside tree (the root is the tree's last 32 bytes)");
    const gpu_info& gpu = select_gpu((int)device_id);

    merkle_call c;
    c.elem_bytes = sizeof(fr_t); c.lg_n = lg_n; c.width = width; c.layout = m.layout; c.hash = hash;
    c.cus = (unsigned)gpu.prop.multiProcessorCount;
    const merkle_route route = make_merkle_route(c);
    if (route.invalid) reject(who + ": no route");

    const bool root_dev = root != nullptr && is_device_pointer(root), root_aligned = ((uintptr_t)root & 15) == 0;
    call_scope sc(s);
    const void* d_in = merkle_matrix_in(sc, in, m);
    mk_digest* d_tree = (mk_digest*)sc.out<char>(tree, tree_bytes);
    mk_digest* d_root = root_dev && root_aligned ? (mk_digest*)root : nullptr;     // (the kernel writes an aligned device root itself)
    if (hash == MERKLE_BLAKE2S) merkle_run<MERKLE_BLAKE2S>(route, d_tree, d_root, d_in, m, lg_n, s);
    else                        merkle_run<MERKLE_SHA256>(route, d_tree, d_root, d_in, m, lg_n, s);
    const char* top = (const char*)d_tree + tree_bytes - sizeof(mk_digest);
    if (root != nullptr && !root_dev) sc.copy_out(root, top, sizeof(mk_digest));
    else if (root != nullptr && d_root == nullptr) HIP_OK(hipMemcpyAsync(root, top, sizeof(mk_digest), hipMemcpyDefault, s));
    sc.finish();                        // (everything on the device and a stream: only enqueued)
}

unsigned merkle_gather_grid(const gpu_info& gpu, size_t items)
{
    const size_t cap = (size_t)std::max(gpu.prop.multiProcessorCount, 1) * MERKLE_WG_PER_CU;
    return (unsigned)std::min(std::max<size_t>((items + MERKLE_NT - 1) / MERKLE_NT, 1), cap);
}

void merkle_open_any(size_t device_id, void* paths, const void* tree, uint32_t lg_n, const uint64_t* indices, size_t nidx, hipStream_t s)
{
    const std::string who("sppark_merkle_open");
    if (paths == nullptr || tree == nullptr) reject(who + ": NULL buffer");
    if (lg_n > MERKLE_MAX_LG) reject(who + ": lg_n above " + std::to_string(MERKLE_MAX_LG));
    if (((uintptr_t)tree | (uintptr_t)paths) & 15) reject(who + ": misaligned tree or paths (16 bytes)");
    const size_t bytes = checked_mul(checked_mul(nidx, lg_n, who.c_str(), MERKLE_OVERFLOW), sizeof(mk_digest), who.c_str(), MERKLE_OVERFLOW);
    (void)checked_mul(nidx, sizeof(uint64_t), who.c_str(), MERKLE_OVERFLOW);
    merkle_check_indices(indices, nidx, lg_n, who);
    const size_t tree_bytes = (((size_t)2 << lg_n) - 1) * sizeof(mk_digest);
    if (bytes && ranges_meet(paths, bytes, tree, tree_bytes)) reject(who + ": paths may not overlap tree");
    if (bytes == 0) return;                                                 // lg_n == 0 or no query: nothing to write
    const gpu_info& gpu = select_gpu((int)device_id);

    const size_t pieces = bytes / sizeof(mk_q);
    if (!is_device_pointer(tree)) {                                         // a tree on the host is read where it lies
        std::vector<mk_q> got(pieces);
        for (size_t g = 0; g < pieces; g++) merkle_open_item(got.data(), (const mk_q*)tree, lg_n, indices, g);
        HIP_OK(hipMemcpyAsync(paths, got.data(), bytes, hipMemcpyDefault, s));
        HIP_OK(hipStreamSynchronize(s));
        return;
    }
    call_scope sc(s);
    const uint64_t* d_idx = sc.in<uint64_t>(indices, nidx);
    mk_q* d_paths = (mk_q*)sc.out<char>(paths, bytes);
    hipLaunchKernelGGL(k_merkle_open, dim3(merkle_gather_grid(gpu, pieces)), dim3(MERKLE_NT), 0, s, d_paths, (const mk_q*)tree, lg_n, d_idx, pieces);
    HIP_OK(hipGetLastError());
    sc.finish(true);
}

void merkle_gather_any(size_t device_id, void* rows, const void* in, uint32_t lg_n, size_t width, size_t col_stride, size_t leaf_stride,
                       const uint64_t* indices, size_t nidx, hipStream_t s)
{
    const std::string who("sppark_merkle_gather");
    if (rows == nullptr) reject(who + ": NULL rows");
    const merkle_matrix m = merkle_matrix_of(in, lg_n, width, col_stride, leaf_stride, who);
    const size_t nwords = checked_mul(checked_mul(nidx, width, who.c_str(), MERKLE_OVERFLOW), MERKLE_EW, who.c_str(), MERKLE_OVERFLOW);
    const size_t bytes = checked_mul(nwords, 4, who.c_str(), MERKLE_OVERFLOW);
    (void)checked_mul(nidx, sizeof(uint64_t), who.c_str(), MERKLE_OVERFLOW);
    merkle_check_indices(indices, nidx, lg_n, who);
    if ((uintptr_t)rows & 3) reject(who + ": misaligned rows");
    if (bytes && ranges_meet(rows, bytes, in, m.span_bytes)) reject(who + ": rows may not overlap in");
    if (bytes == 0) return;
    const gpu_info& gpu = select_gpu((int)device_id);

    if (!is_device_pointer(in)) {                                           // a matrix on the host is read where it lies
        std::vector<u32> got(nwords);
        for (size_t g = 0; g < nwords; g++) merkle_gather_item(got.data(), (const u32*)in, width, col_stride, leaf_stride, MERKLE_EW, indices, g);
        HIP_OK(hipMemcpyAsync(rows, got.data(), bytes, hipMemcpyDefault, s));
        HIP_OK(hipStreamSynchronize(s));
        return;
    }
    call_scope sc(s);
    const uint64_t* d_idx = sc.in<uint64_t>(indices, nidx);
    u32* d_rows = sc.out<u32>(rows, nwords);
    hipLaunchKernelGGL(k_merkle_gather, dim3(merkle_gather_grid(gpu, nwords)), dim3(MERKLE_NT), 0, s, d_rows, (const u32*)in, width,
                       col_stride, leaf_stride, MERKLE_EW, d_idx, nwords);
    HIP_OK(hipGetLastError());
    sc.finish(true);
}
}

SPPARK_FFI RustError sppark_merkle_commit(size_t device_id, void* tree, void* root, const void* in, uint32_t lg_n, size_t width,
                                          size_t col_stride, size_t leaf_stride, int hash, void* stream)
{   return guarded([&] { merkle_commit_any(device_id, tree, root, in, lg_n, width, col_stride, leaf_stride, hash, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_merkle_open(size_t device_id, void* paths, const void* tree, uint32_t lg_n, const uint64_t* indices, size_t nidx,
                                        void* stream)
{   return guarded([&] { merkle_open_any(device_id, paths, tree, lg_n, indices, nidx, (hipStream_t)stream); });   }

SPPARK_FFI RustError sppark_merkle_gather(size_t device_id, void* rows, const void* in, uint32_t lg_n, size_t width, size_t col_stride,
                                          size_t leaf_stride, const uint64_t* indices, size_t nidx, void* stream)
{
    return guarded([&] { merkle_gather_any(device_id, rows, in, lg_n, width, col_stride, leaf_stride, indices, nidx, (hipStream_t)stream); });
}
