// C entry points of the Merkle commitments over matrices of the library's field fr_t (include/sppark_amd_merkle.h).
// Included behind api/mle_api.hpp, whose argument checks (field_reject, vec_ranges_meet) it shares.  The launches are those
// of merkle/merkle_route.hpp: the driver below runs what the route says.  The kernels see the elements as sizeof(fr_t) / 4
// opaque words.
// Expects: fr_t, guarded(), SPPARK_FFI, select_gpu, is_device_pointer in scope.
#pragma once
#include "mle_api.hpp"
#include "../merkle/merkle_kernels.hpp"
#include <vector>

namespace {
constexpr unsigned MERKLE_EW = sizeof(fr_t) / 4;
static_assert(sizeof(fr_t) == 4 || sizeof(fr_t) == 8 || sizeof(fr_t) == 16 || sizeof(fr_t) == 32, "elements of 1, 2, 4 or 8 words");

size_t merkle_mul(size_t a, size_t b, const std::string& who)
{
    size_t r = 0;
    if (__builtin_mul_overflow(a, b, &r)) field_reject((who + ": a size overflows size_t").c_str());
    return r;
}
size_t merkle_add(size_t a, size_t b, const std::string& who)
{
    size_t r = 0;
    if (__builtin_add_overflow(a, b, &r)) field_reject((who + ": a size overflows size_t").c_str());
    return r;
}

struct merkle_matrix { size_t n, width, col_stride, leaf_stride, span_bytes; int layout; };

// the matrix arguments of commit and gather: the layout and the bytes from the first element to the end of the last
merkle_matrix merkle_matrix_of(const void* in, uint32_t lg_n, size_t width, size_t col_stride, size_t leaf_stride, const std::string& who)
{
    if (in == nullptr) field_reject((who + ": NULL in").c_str());
    if (lg_n > MERKLE_MAX_LG) field_reject((who + ": lg_n above " + std::to_string(MERKLE_MAX_LG)).c_str());
    if (width == 0) field_reject((who + ": width == 0").c_str());
    if (width > (size_t)0xffffffffu / sizeof(fr_t)) field_reject((who + ": width * sizeof(element) reaches 2^32").c_str());
    merkle_matrix m;
    m.n = (size_t)1 << lg_n; m.width = width; m.col_stride = col_stride; m.leaf_stride = leaf_stride;
    if (leaf_stride == 1 && col_stride >= m.n) m.layout = MERKLE_COLUMNS;
    else if (col_stride == 1 && leaf_stride >= width) m.layout = MERKLE_ROWS;
    else field_reject((who + ": strides are neither columns (leaf_stride == 1, col_stride >= n) nor rows (col_stride == 1, leaf_stride >= width)").c_str());
    const size_t last = merkle_add(merkle_mul(width - 1, col_stride, who), merkle_mul(m.n - 1, leaf_stride, who), who);
    m.span_bytes = merkle_mul(merkle_add(last, 1, who), sizeof(fr_t), who);
    if ((uintptr_t)in % (sizeof(fr_t) < 16 ? sizeof(fr_t) : 16)) field_reject((who + ": misaligned in").c_str());
    return m;
}

void merkle_check_indices(const uint64_t* indices, size_t nidx, uint32_t lg_n, const std::string& who)
{
    if (nidx && indices == nullptr) field_reject((who + ": NULL indices with nidx > 0").c_str());
    for (size_t q = 0; q < nidx; q++)
        if (indices[q] >> lg_n) field_reject((who + ": index " + std::to_string(q) + " is not below n").c_str());
}

// a compact device copy of a host matrix: only the elements are read, never the gaps of a stride
struct merkle_staged_matrix {
    pooled_scratch buf;
    merkle_staged_matrix(const void* in, merkle_matrix& m, hipStream_t s) : buf(m.n * m.width * sizeof(fr_t))
    {
        const bool cols = m.layout == MERKLE_COLUMNS;
        const size_t line = (cols ? m.n : m.width) * sizeof(fr_t), lines = cols ? m.width : m.n;
        const size_t pitch = (cols ? m.col_stride : m.leaf_stride) * sizeof(fr_t);
        if (pitch == line) HIP_OK(hipMemcpyAsync(buf.p, in, line * lines, hipMemcpyHostToDevice, s));
        else HIP_OK(hipMemcpy2DAsync(buf.p, line, in, pitch, line, lines, hipMemcpyHostToDevice, s));
        if (cols) m.col_stride = m.n; else m.leaf_stride = m.width;
    }
};

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
    if (tree == nullptr) field_reject((who + ": NULL tree").c_str());
    merkle_matrix m = merkle_matrix_of(in, lg_n, width, col_stride, leaf_stride, who);
    if (hash != MERKLE_BLAKE2S && hash != MERKLE_SHA256) field_reject((who + ": unknown hash").c_str());
    if ((uintptr_t)tree & 15) field_reject((who + ": misaligned tree (16 bytes)").c_str());
    const size_t tree_bytes = (((size_t)2 << lg_n) - 1) * sizeof(mk_digest);
    if (vec_ranges_meet(tree, tree_bytes, in, m.span_bytes)) field_reject((who + ": tree may not overlap in").c_str());
    if (root != nullptr && vec_ranges_meet(root, sizeof(mk_digest), in, m.span_bytes)) field_reject((who + ": root may not overlap in").c_str());
    if (root != nullptr && vec_ranges_meet(root, sizeof(mk_digest), tree, tree_bytes))
        field_reject((who + ": root may not lie inside tree (the root is the tree's last 32 bytes)").c_str());
    const gpu_info& gpu = select_gpu((int)device_id);

    merkle_call c;
    c.elem_bytes = sizeof(fr_t); c.lg_n = lg_n; c.width = width; c.layout = m.layout; c.hash = hash;
    c.cus = (unsigned)gpu.prop.multiProcessorCount;
    const merkle_route route = make_merkle_route(c);
    if (route.invalid) field_reject((who + ": no route").c_str());

    const bool in_dev = is_device_pointer(in), tree_dev = is_device_pointer(tree), root_dev = root != nullptr && is_device_pointer(root);
    const bool root_aligned = ((uintptr_t)root & 15) == 0;
    std::unique_ptr<merkle_staged_matrix> vin;
    std::unique_ptr<pooled_scratch> vtree;
    const void* d_in = in;
    if (!in_dev) { vin.reset(new merkle_staged_matrix(in, m, s)); d_in = vin->buf.p; }
    if (!tree_dev) vtree.reset(new pooled_scratch(tree_bytes));
    mk_digest* d_tree = tree_dev ? (mk_digest*)tree : (mk_digest*)vtree->p;
    mk_digest* d_root = root_dev && root_aligned ? (mk_digest*)root : nullptr;     // (the kernel writes an aligned device root itself)
    if (hash == MERKLE_BLAKE2S) merkle_run<MERKLE_BLAKE2S>(route, d_tree, d_root, d_in, m, lg_n, s);
    else                        merkle_run<MERKLE_SHA256>(route, d_tree, d_root, d_in, m, lg_n, s);
    if (root != nullptr && d_root == nullptr)
        HIP_OK(hipMemcpyAsync(root, (const char*)d_tree + tree_bytes - sizeof(mk_digest), sizeof(mk_digest), hipMemcpyDefault, s));
    if (in_dev && tree_dev && (root == nullptr || root_dev) && s != nullptr) return;            // only enqueued
    if (!tree_dev) HIP_OK(hipMemcpyAsync(tree, d_tree, tree_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (vin) vin->buf.done();
    if (vtree) vtree->done();
}

// the indices on the device, the result either in the caller's device buffer or in scratch that goes back to the host
struct merkle_query {
    pooled_scratch idx;
    std::unique_ptr<pooled_scratch> out;
    void* d_out; void* host_out = nullptr; size_t out_bytes;
    merkle_query(const uint64_t* indices, size_t nidx, void* result, size_t bytes, hipStream_t s) : idx(nidx * sizeof(uint64_t)), out_bytes(bytes)
    {
        HIP_OK(hipMemcpyAsync(idx.p, indices, nidx * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        if (is_device_pointer(result)) d_out = result;
        else { out.reset(new pooled_scratch(bytes)); d_out = out->p; host_out = result; }
    }
    void finish(hipStream_t s)
    {
        if (host_out) HIP_OK(hipMemcpyAsync(host_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        idx.done();
        if (out) out->done();
    }
};
unsigned merkle_gather_grid(const gpu_info& gpu, size_t items)
{
    const size_t cap = (size_t)std::max(gpu.prop.multiProcessorCount, 1) * MERKLE_WG_PER_CU;
    return (unsigned)std::min(std::max<size_t>((items + MERKLE_NT - 1) / MERKLE_NT, 1), cap);
}

void merkle_open_any(size_t device_id, void* paths, const void* tree, uint32_t lg_n, const uint64_t* indices, size_t nidx, hipStream_t s)
{
    const std::string who("sppark_merkle_open");
    if (paths == nullptr || tree == nullptr) field_reject((who + ": NULL buffer").c_str());
    if (lg_n > MERKLE_MAX_LG) field_reject((who + ": lg_n above " + std::to_string(MERKLE_MAX_LG)).c_str());
    if (((uintptr_t)tree | (uintptr_t)paths) & 15) field_reject((who + ": misaligned tree or paths (16 bytes)").c_str());
    const size_t bytes = merkle_mul(merkle_mul(nidx, lg_n, who), sizeof(mk_digest), who);
    (void)merkle_mul(nidx, sizeof(uint64_t), who);
    merkle_check_indices(indices, nidx, lg_n, who);
    const size_t tree_bytes = (((size_t)2 << lg_n) - 1) * sizeof(mk_digest);
    if (bytes && vec_ranges_meet(paths, bytes, tree, tree_bytes)) field_reject((who + ": paths may not overlap tree").c_str());
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
    merkle_query q(indices, nidx, paths, bytes, s);
    hipLaunchKernelGGL(k_merkle_open, dim3(merkle_gather_grid(gpu, pieces)), dim3(MERKLE_NT), 0, s, (mk_q*)q.d_out, (const mk_q*)tree, lg_n,
                       (const uint64_t*)q.idx.p, pieces);
    HIP_OK(hipGetLastError());
    q.finish(s);
}

void merkle_gather_any(size_t device_id, void* rows, const void* in, uint32_t lg_n, size_t width, size_t col_stride, size_t leaf_stride,
                       const uint64_t* indices, size_t nidx, hipStream_t s)
{
    const std::string who("sppark_merkle_gather");
    if (rows == nullptr) field_reject((who + ": NULL rows").c_str());
    const merkle_matrix m = merkle_matrix_of(in, lg_n, width, col_stride, leaf_stride, who);
    const size_t nwords = merkle_mul(merkle_mul(nidx, width, who), MERKLE_EW, who), bytes = merkle_mul(nwords, 4, who);
    (void)merkle_mul(nidx, sizeof(uint64_t), who);
    merkle_check_indices(indices, nidx, lg_n, who);
    if ((uintptr_t)rows & 3) field_reject((who + ": misaligned rows").c_str());
    if (bytes && vec_ranges_meet(rows, bytes, in, m.span_bytes)) field_reject((who + ": rows may not overlap in").c_str());
    if (bytes == 0) return;
    const gpu_info& gpu = select_gpu((int)device_id);

    if (!is_device_pointer(in)) {                                           // a matrix on the host is read where it lies
        std::vector<u32> got(nwords);
        for (size_t g = 0; g < nwords; g++) merkle_gather_item(got.data(), (const u32*)in, width, col_stride, leaf_stride, MERKLE_EW, indices, g);
        HIP_OK(hipMemcpyAsync(rows, got.data(), bytes, hipMemcpyDefault, s));
        HIP_OK(hipStreamSynchronize(s));
        return;
    }
    merkle_query q(indices, nidx, rows, bytes, s);
    hipLaunchKernelGGL(k_merkle_gather, dim3(merkle_gather_grid(gpu, nwords)), dim3(MERKLE_NT), 0, s, (u32*)q.d_out, (const u32*)in, width,
                       col_stride, leaf_stride, MERKLE_EW, (const uint64_t*)q.idx.p, nwords);
    HIP_OK(hipGetLastError());
    q.finish(s);
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
