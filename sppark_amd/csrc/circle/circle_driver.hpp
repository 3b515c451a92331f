// Driver of the circle transform over Mersenne31: fetches and caches the tables and launches the steps
// make_circle_route returns (circle_route.hpp), one launch group after the other when the batch exceeds the grid's
// y limit.  Mirrors ntt_engine::run (ntt/ntt_driver.hpp).
//
// Tables per device: the 4096 points of circle_gpow (32 KB, every forward transform) and the inverse twiddles L_m / Y_m
// for m <= circle_knobs::cache_max_lg, built on first use (one field inversion per entry, ~60 products; the stream
// is synchronised after a build, before the tables enter the cache, so that other threads and streams only find complete ones).  Larger inverse tables are
// built into the scratch pool's buffer for the call and given back: at most 2^lg elements, whatever the batch.
#pragma once
#include "circle_kernels.hpp"
#include "circle_route.hpp"
#include "../util/runtime.hpp"
#include <map>
#include <memory>
#include <mutex>
#include <utility>

namespace sppark_amd {

extern template __global__ void k_circle_pass<false>(cf_t*, size_t, size_t, circle_pass, const circle_pt*);
extern template __global__ void k_circle_pass<true>(cf_t*, size_t, size_t, circle_pass, const circle_pt*);

struct circle_engine {
    struct dev_state {
        circle_pt* pts = nullptr;
        std::map<std::pair<unsigned, bool>, cf_t*> inv;
        size_t bytes = 0;
    };
    std::mutex mtx;
    std::map<int, dev_state> devs;
    static circle_engine& instance() { static circle_engine e; return e; }
    static const circle_knobs& knobs() { static const circle_knobs k; return k; }

    size_t cached_bytes(int hip_dev)
    {
        std::lock_guard<std::mutex> lk(mtx);
        auto it = devs.find(hip_dev);
        return it == devs.end() ? 0 : it->second.bytes;
    }
    // Frees the device's tables.  NOT to be called while another thread runs a transform on that device: such a call may
    // hold table pointers it has not launched with yet, which the device-wide wait below cannot see (the header says so).
    void release(int hip_dev)
    {
        std::lock_guard<std::mutex> lk(mtx);
        auto it = devs.find(hip_dev);
        if (it == devs.end()) return;
        HIP_OK(hipDeviceSynchronize());                 // (no kernel may still read a table)
        if (it->second.pts) (void)hipFree(it->second.pts);
        for (auto& kv : it->second.inv) (void)hipFree(kv.second);
        devs.erase(it);
    }

    static void build_inv_table(cf_t* out, const circle_pt* pts, unsigned m, bool y, hipStream_t stream)
    {
        const size_t count = (size_t)1 << (m - 2);
        hipLaunchKernelGGL(k_circle_inv_table<circle_pt>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, out, pts, m, y ? 1 : 0);
        HIP_OK(hipGetLastError());
    }
    // the point tables of this device (built on first use)
    const circle_pt* points(int hip_dev, hipStream_t stream)
    {
        std::lock_guard<std::mutex> lk(mtx);
        dev_state& d = devs[hip_dev];
        if (d.pts) return d.pts;
        circle_pt* p = nullptr;
        HIP_OK(dev_scratch_pool::malloc_or_drain((void**)&p, CIRCLE_PT_ENTRIES * sizeof(circle_pt)));
        hipLaunchKernelGGL(k_circle_points<circle_pt>, dim3(CIRCLE_PT_ENTRIES / 256), dim3(256), 0, stream, p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { (void)hipFree(p); HIP_OK(e); }
        d.pts = p; d.bytes += CIRCLE_PT_ENTRIES * sizeof(circle_pt);
        return p;
    }
    // The cached tables a route asks for, into tabs[] (entries of uncached requests are left alone).  Missing ones are built
    // on |stream| and the stream is synchronised BEFORE they enter the cache, under the lock: a table must be complete
    // before another thread can find it (ntt_engine::tables does the same).  A failure frees what this call built and
    // leaves the cache as it was.  Returns true when it built (and so synchronised).
    bool cached_tables(int hip_dev, const circle_pt* pts, const circle_route& r, const cf_t** tabs, hipStream_t stream)
    {
        std::lock_guard<std::mutex> lk(mtx);
        dev_state& d = devs[hip_dev];
        unsigned fresh[circle_route::TCAP], nfresh = 0;
        cf_t* mem[circle_route::TCAP] = {};
        hipError_t e = hipSuccess;
        for (unsigned i = 0; i < r.ntables && e == hipSuccess; i++) {
            const circle_table_req& q = r.tables[i];
            if (!q.cached) continue;
            auto it = d.inv.find(std::make_pair(q.m, q.y));
            if (it != d.inv.end()) { tabs[i] = it->second; continue; }
            e = dev_scratch_pool::malloc_or_drain((void**)&mem[nfresh], q.count * sizeof(cf_t));
            if (e != hipSuccess) break;
            fresh[nfresh++] = i;
            hipLaunchKernelGGL(k_circle_inv_table<circle_pt>, dim3((unsigned)((q.count + 255) / 256)), dim3(256), 0, stream,
                               mem[nfresh - 1], pts, q.m, q.y ? 1 : 0);
            e = hipGetLastError();
        }
        if (nfresh == 0 && e == hipSuccess) return false;
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(stream);                 // (no build kernel may still write what is freed)
            for (unsigned j = 0; j < nfresh; j++) (void)hipFree(mem[j]);
            HIP_OK(e);
        }
        for (unsigned j = 0; j < nfresh; j++) {
            const circle_table_req& q = r.tables[fresh[j]];
            d.inv[std::make_pair(q.m, q.y)] = mem[j]; d.bytes += q.count * sizeof(cf_t);
            tabs[fresh[j]] = mem[j];
        }
        return true;
    }

    static void launch_bitrev(const circle_step& s, cf_t* d, size_t stride, hipStream_t stream)
    {
        constexpr unsigned TB = bitrev_tile_bits<cf_t>::value;
        static_assert(TB == CIRCLE_BITREV_TILE_BITS, "circle_route.hpp sizes the tiled bit reversal's grid and LDS for this tile edge");
        const dim3 grid(s.gx, s.gy), block(s.block);
        if (s.kernel == CK_BITREV) hipLaunchKernelGGL(k_bitrev<cf_t>, grid, block, 0, stream, d, s.lg, stride);
        else if (s.kernel == CK_BITREV_TILED) hipLaunchKernelGGL((k_bitrev_tiled<cf_t, TB>), grid, block, s.lds, stream, d, s.lg, stride);
        else hipLaunchKernelGGL((k_bitrev_tiled_vec<cf_t, TB>), grid, block, s.lds, stream, d, s.lg, stride);
    }

    // |batch| in-place transforms of 2^lg elements, column j at d + j * stride.  Returns true when it synchronised the stream.
    bool run(const gpu_info& gpu, cf_t* d, unsigned lg, size_t batch, size_t stride, int order, int direction, hipStream_t stream,
             unsigned pad_lg = 32)
    {
        if (lg == 0 || batch == 0) return false;
        circle_call c;
        c.lg = lg; c.order = order; c.direction = direction; c.batch = batch; c.pad_lg = pad_lg;
        c.max_grid_y = (size_t)std::max(gpu.prop.maxGridSize[1], 1);
        c.aligned16 = ((uintptr_t)d % 16 == 0) && (batch == 1 || stride % 4 == 0);
        bool synced = false;
        for (size_t c0 = 0; c0 < batch; ) {
            c.batch = batch - c0;
            const circle_route r = make_circle_route(knobs(), c);
            if (r.invalid || r.cols == 0) HIP_OK(hipErrorInvalidValue);
            const circle_pt* pts = points(gpu.hip_id, stream);          // (the inverse tables are built from them too)
            const cf_t* tabs[circle_route::TCAP] = {};
            if (cached_tables(gpu.hip_id, pts, r, tabs, stream)) synced = true;
            std::unique_ptr<pooled_scratch> scratch;
            if (r.scratch_entries) scratch.reset(new pooled_scratch(r.scratch_entries * sizeof(cf_t)));
            size_t off = 0;
            for (unsigned i = 0; i < r.ntables; i++) {
                const circle_table_req& q = r.tables[i];
                if (q.cached) continue;                                 // (the call's own tables: same stream, no one else sees them)
                cf_t* t = (cf_t*)scratch->p + off;
                off += q.count;
                build_inv_table(t, pts, q.m, q.y, stream);
                tabs[i] = t;
            }
            cf_t* base = d + c0 * stride;
            for (unsigned i = 0; i < r.nsteps; i++) {
                const circle_step& s = r.steps[i];
                if (s.kernel != CK_PASS) { launch_bitrev(s, base, stride, stream); continue; }
                circle_pass P;
                P.k = s.lg; P.b_lo = s.b_lo; P.S = s.S; P.lgC = s.lgC; P.lgT = s.lgT; P.vec = s.vec; P.pad_lg = s.pad_lg;
                P.scale = s.scales ? scale_of(s.lg) : 0;
                for (unsigned lb = 0; lb < CIRCLE_MAX_S; lb++) P.itw[lb] = s.table[lb] >= 0 ? tabs[s.table[lb]] : nullptr;
                const dim3 grid(s.gx, s.gy), block(s.block);
                if (s.inverse) hipLaunchKernelGGL(k_circle_pass<true>, grid, block, s.lds, stream, base, stride, r.cols, P, pts);
                else           hipLaunchKernelGGL(k_circle_pass<false>, grid, block, s.lds, stream, base, stride, r.cols, P, pts);
            }
            HIP_OK(hipGetLastError());
            if (scratch) { HIP_OK(hipStreamSynchronize(stream)); scratch->done(); synced = true; }
            c0 += r.cols;
        }
        return synced;
    }
    // 1 / 2^lg mod p: 2^31 = 1, so 2^(31 - lg)
    static u32 scale_of(unsigned lg) { return lg == 0 ? 1u : 1u << (31 - lg); }

    // |batch| low-degree extensions: column j owns d[j * ext, (j + 1) * ext), its first 2^lg elements hold the evaluations on
    // D_lg; on return the evaluations on D_{lg + lg_blowup} in the same order.  d_aux: null or batch x 2^lg coefficients.
    void lde(const gpu_info& gpu, cf_t* d, unsigned lg, unsigned lg_blowup, size_t batch, int order, cf_t* d_aux, hipStream_t stream)
    {
        if (batch == 0) return;
        const size_t dom = (size_t)1 << lg, ext = (size_t)1 << (lg + lg_blowup);
        run(gpu, d, lg, batch, ext, order, CIRCLE_INVERSE, stream);
        if (d_aux) {
            if (batch == 1) HIP_OK(hipMemcpyAsync(d_aux, d, dom * sizeof(cf_t), hipMemcpyDeviceToDevice, stream));
            else HIP_OK(hipMemcpy2DAsync(d_aux, dom * sizeof(cf_t), d, ext * sizeof(cf_t), dom * sizeof(cf_t), batch, hipMemcpyDeviceToDevice, stream));
        }
        if (lg_blowup == 0) { run(gpu, d, lg, batch, ext, order, CIRCLE_FORWARD, stream); return; }
        // (the zero padding rides in the first forward pass's load: nothing above 2^lg is read)
        run(gpu, d, lg + lg_blowup, batch, ext, order, CIRCLE_FORWARD, stream, lg);
    }
};

} // namespace sppark_amd
