// C-ABI of the MSM library (one .so per curve, selected by -DFEATURE_*, as the
// reference's poc/msm-cuda/build.rs does).  Declarations + reference
// citations: include/sppark_amd.h.  No C++ exception crosses this boundary
// (msm/pippenger.cuh:735-746).
#include "../msm/curve_select.hpp"
#include "../msm/msm_kernels.hpp"
#include "../msm/msm_coop_kernels.hpp"
#include "../msm/msm_g2c_kernels.hpp"
#include "../msm/msm_sort_kernels.hpp"

// the big kernels are instantiated in their own translation units
// (msm/k_accumulate.hip, k_reduce.hip, k_bucket1.hip, k_bucketN.hip)
namespace sppark_amd {
extern template __global__ void k_accumulate<msm_fp_d, false>(bucket_m*, u32*, bucket_m*, const unsigned char*, unsigned,
                                                          const u32*, const u32*, unsigned, unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_accumulate<msm_fp_d, true>(bucket_m*, u32*, bucket_m*, const unsigned char*, unsigned,
                                                         const u32*, const u32*, unsigned, unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bitmap_accumulate<msm_fp_d, false>(u32*, bucket_m*, const unsigned char*, unsigned, unsigned, const u32*, const u32*, unsigned);
extern template __global__ void k_bitmap_accumulate<msm_fp_d, true>(u32*, bucket_m*, const unsigned char*, unsigned, unsigned, const u32*, const u32*, unsigned);
extern template __global__ void k_reduce_runs<msm_fp_d>(bucket_m*, u32*, bucket_m*, const u32*, const bucket_m*,
                                                    unsigned, unsigned, unsigned, int, const u32*);
extern template __global__ void k_join_runs<msm_fp_d>(bucket_m*, u32*, const u32*, const bucket_m*, unsigned, u32*);
extern template __global__ void k_reduce_tail<msm_fp_d>(bucket_m*, u32*, bucket_m*, u32*, bucket_m*, unsigned, unsigned, const u32*);
extern template __global__ void k_piece_level<msm_fp_d>(bucket_m*, u32*, bucket_m*, const u32*, unsigned, unsigned, unsigned, unsigned,
                                                        unsigned, unsigned, unsigned, u32*);
extern template __global__ void k_bucket_levelN_pipe<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_level1_pipe<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_small_bits_coop<msm_fp_d>(bucket_m*, const bucket_m*, const u32*, unsigned, unsigned);
extern template __global__ void k_piece_level_coop<msm_fp_d>(bucket_m*, u32*, bucket_m*, const u32*, unsigned, unsigned, unsigned, unsigned,
                                                             unsigned, unsigned, unsigned, u32*);
extern template __global__ void k_piece_tail_coop<msm_fp_d>(bucket_m*, u32*, bucket_m*, const u32*, unsigned, unsigned, unsigned, unsigned,
                                                            unsigned, unsigned, unsigned, u32*);
extern template __global__ void k_bucket_level1<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_levelN<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, const bucket_m*,
                                                      unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_level1_lat<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_levelN_lat<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, const bucket_m*,
                                                          unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_bits<msm_fp_d>(bucket_m*, const bucket_m*, const bucket_m*, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_bits_coop<msm_fp_d>(bucket_m*, const bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_sum_coop<msm_fp_d>(bucket_m*, const bucket_m*, unsigned, xyzz_mem<msm_fp_d::NW>*, u32*, u32*);
extern template __global__ void k_reduce_runs_coop<msm_fp_d>(bucket_m*, u32*, bucket_m*, const u32*, const bucket_m*,
                                                         unsigned, unsigned, unsigned, int, const u32*);
extern template __global__ void k_reduce_tail_coop<msm_fp_d>(bucket_m*, u32*, bucket_m*, u32*, bucket_m*, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_level1_coop<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, unsigned, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_levelN_coop<msm_fp_d>(bucket_m*, bucket_m*, const bucket_m*, const bucket_m*,
                                                           unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_sum<msm_fp_d>(bucket_m*, const bucket_m*, unsigned);
// ... and once more over Fp2 for G2 (the same units compiled with -DSPPARK_G2)
#ifndef SPPARK_NO_G2
extern template __global__ void k_accumulate<fp2_d, false>(bucket2_m*, u32*, bucket2_m*, const unsigned char*, unsigned,
                                                           const u32*, const u32*, unsigned, unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_accumulate<fp2_d, true>(bucket2_m*, u32*, bucket2_m*, const unsigned char*, unsigned,
                                                          const u32*, const u32*, unsigned, unsigned, unsigned, unsigned, unsigned);
#if !defined(SPPARK_FP2_32LIMB)
extern template __global__ void k_accumulate_g2c<fp2_d>(bucket2_m*, u32*, bucket2_m*, const unsigned char*, unsigned,
                                                               const u32*, const u32*, unsigned, unsigned, unsigned, unsigned, unsigned);
#endif
extern template __global__ void k_reduce_runs<fp2_d>(bucket2_m*, u32*, bucket2_m*, const u32*, const bucket2_m*,
                                                     unsigned, unsigned, unsigned, int, const u32*);
extern template __global__ void k_join_runs<fp2_d>(bucket2_m*, u32*, const u32*, const bucket2_m*, unsigned, u32*);
extern template __global__ void k_reduce_tail<fp2_d>(bucket2_m*, u32*, bucket2_m*, u32*, bucket2_m*, unsigned, unsigned, const u32*);
extern template __global__ void k_piece_level<fp2_d>(bucket2_m*, u32*, bucket2_m*, const u32*, unsigned, unsigned, unsigned, unsigned,
                                                     unsigned, unsigned, unsigned, u32*);
extern template __global__ void k_bucket_level1<fp2_d>(bucket2_m*, bucket2_m*, const bucket2_m*, unsigned, unsigned, unsigned, const u32*);
extern template __global__ void k_bucket_levelN<fp2_d>(bucket2_m*, bucket2_m*, const bucket2_m*, const bucket2_m*,
                                                       unsigned, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_bits<fp2_d>(bucket2_m*, const bucket2_m*, const bucket2_m*, unsigned, unsigned, unsigned);
extern template __global__ void k_bucket_top_sum<fp2_d>(bucket2_m*, const bucket2_m*, unsigned);
#endif
}

#include "../ff/fp2_host.hpp"
#include "../msm/msm_driver.hpp"
#include "common_api.hpp"
#include "../util/rccl_dyn.hpp"
#include <chrono>
#include <map>
#include <memory>

using namespace sppark_amd;

typedef msm_t<msm_fp_d, mont_host<curve_p::fp>, curve_p::fr> msm_impl;
typedef msm_impl::point_t point_t;
typedef msm_impl::fp_h fp_h;
#ifndef SPPARK_NO_G2                     // (the Pasta curves have no pairing and no G2)
typedef msm_t<fp2_d, fp2_host<curve_p::fp>, curve_p::fr> msm2_impl;       // G2
typedef msm2_impl::point_t point2_t;
typedef msm2_impl::fp_h fp2_h;
#endif

struct sppark_msm_ctx { msm_impl impl; sppark_msm_ctx(int id, hipStream_t s) : impl(id, s) {} };

static void store_point(void* out, const point_t& p) { memcpy(out, &p, sizeof(p)); }
static void store_inf(void* out) { memset(out, 0, sizeof(point_t)); }

// The reference's entry points build an msm_t per call (msm/pippenger.cuh:730-747), i.e. a device
// allocation and release of the whole scratch every time.  With GBs of scratch that costs up to
// 100+ ms per call on a busy device, so the one-shot entry points borrow a context from a
// PROCESS-WIDE pool keyed by device (not thread-local: a caller that runs every proof on a fresh
// thread must not strand one scratch blob per dead thread) and give it back after the call.  A
// returned context keeps its scratch only while it is below the cache limit
// (SPPARK_MSM_CACHE_BYTES, default 32 GiB); sppark_msm_release_cached() frees the scratch of
// every idle context.  The pool itself is never destroyed: destructors running HIP calls at
// process exit would race the runtime's own teardown.
#include <atomic>
#include <mutex>
#include <thread>
template<class Impl> class ctx_pool {
    std::mutex mtx;
    std::multimap<int, Impl*> idle;         // HIP device ordinal -> idle contexts
    static size_t cache_limit()
    {
        static const size_t lim = [] {
            const char* e = getenv("SPPARK_MSM_CACHE_BYTES");
            return e ? (size_t)strtoull(e, nullptr, 0) : (size_t)32 << 30;
        }();
        return lim;
    }
public:
    static ctx_pool& get() { static ctx_pool* p = new ctx_pool; return *p; }
    // |gid|: index in the filtered device list, -1 = the calling thread's current device
    Impl* take(int gid)
    {
        const gpu_info& g = select_gpu(gid);
        {
            std::lock_guard<std::mutex> lk(mtx);
            auto it = idle.find(g.hip_id);
            if (it != idle.end()) { Impl* c = it->second; idle.erase(it); return c; }
        }
        return new Impl(g.gid);
    }
    void give(Impl* c)
    {
        if (c->scratch_bytes() > cache_limit()) c->release_scratch();
        std::lock_guard<std::mutex> lk(mtx);
        idle.emplace(c->device(), c);
    }
    void release_idle()
    {
        std::lock_guard<std::mutex> lk(mtx);
        int cur = -1;
        (void)hipGetDevice(&cur);
        for (auto& kv : idle) kv.second->release_scratch();
        if (cur >= 0) (void)hipSetDevice(cur);
    }
};
template<class Impl> struct borrowed {      // RAII: back to the pool on every exit path
    Impl* c;
    explicit borrowed(int gid) : c(ctx_pool<Impl>::get().take(gid)) {}
    ~borrowed() { ctx_pool<Impl>::get().give(c); }
    Impl* operator->() { return c; }
};

static RustError one_shot(void* out, const void* points, size_t npoints, const void* scalars,
                          bool mont, size_t ffi_sz)
{
    store_inf(out);
    return guarded([&] {
        borrowed<msm_impl> msm(-1);
        // device-resident inputs may have been produced on ANY stream of the caller: the pooled
        // context's private stream only orders itself after the legacy default stream
        if (is_device_pointer(points) || is_device_pointer(scalars)) HIP_OK(hipDeviceSynchronize());
        point_t r;
        msm->invoke(r, points, npoints, scalars, mont, ffi_sz);
        store_point(out, r);
    });
}

// Multi-GPU MSM inside ONE process (the reference keeps one gpu_t per device in a process,
// util/all_gpus.cpp:39-63, but its msm_t drives a single one): shard i runs on device
// device_ids[i] on its own host thread with a context of its own; the partial results are added
// on the host.  Sum_i s_i*P_i splits over any partition of the index set, so there is exactly
// one exchange step, of 144-byte points.
// |out_ms| (nullable): wall-clock milliseconds of every shard's MSM on its host thread (copies included), so that
// a caller sees load imbalance between the devices.
static void msm_shards(point_t& out, const void* const* points, const size_t* npoints, const void* const* scalars,
                       bool mont, size_t ffi_sz, unsigned nshards, const int* device_ids, float* out_ms = nullptr)
{
    out.set_inf();
    if (nshards == 0) return;
    std::vector<point_t> part(nshards);
    std::vector<RustError> err(nshards, rust_ok());
    auto work = [&](unsigned i) {
        if (out_ms) out_ms[i] = 0.f;
        err[i] = guarded([&] {
            part[i].set_inf();
            if (npoints[i] == 0) return;
            const auto t0 = std::chrono::steady_clock::now();
            borrowed<msm_impl> msm(device_ids ? device_ids[i] : (int)i);    // selects the shard's device
            // device-resident shards may have been produced on ANY stream of that device (as in one_shot())
            if (is_device_pointer(points[i]) || is_device_pointer(scalars[i])) HIP_OK(hipDeviceSynchronize());
            msm->invoke(part[i], points[i], npoints[i], scalars[i], mont, ffi_sz);
            if (out_ms) out_ms[i] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
    };
    int cur = -1;
    (void)hipGetDevice(&cur);
    std::vector<std::thread> threads;
    try {
        for (unsigned i = 1; i < nshards; i++) threads.emplace_back(work, i);
    } catch (...) {                             // thread creation failed: the ones already running must be joined
        for (auto& t : threads) t.join();
        for (auto& e : err) free(e.message);
        if (cur >= 0) (void)hipSetDevice(cur);
        throw;
    }
    work(0);
    for (auto& t : threads) t.join();
    if (cur >= 0) (void)hipSetDevice(cur);      // shard 0 ran on this thread and selected its device
    for (unsigned i = 0; i < nshards; i++)
        if (err[i].code) {
            std::string msg = err[i].message ? err[i].message : "";
            for (auto& e : err) free(e.message);
            throw hip_error(err[i].code, "shard " + std::to_string(i) + ": " + msg);
        }
    for (unsigned i = 0; i < nshards; i++) out.add(part[i]);
}

// the exchange step of the one-process-per-GPU entry points (sppark_msm_rccl_sum below)
template<class Pt> static void rccl_sum(void* out, const void* partial, void* comm, void* stream)
{
    if (!comm || !partial) throw hip_error(EINVAL, "sppark_msm_rccl_sum: null communicator or partial sum");
    const std::vector<unsigned char> all = rccl_all_gather_host(partial, sizeof(Pt), (ncclComm_t)comm, (hipStream_t)stream);
    Pt acc; acc.set_inf();
    for (size_t i = 0; i < all.size() / sizeof(Pt); i++) {
        Pt p; memcpy(&p, all.data() + i * sizeof(Pt), sizeof(p));
        acc.add(p);
    }
    memcpy(out, &acc, sizeof(acc));
}

extern "C" {

SPPARK_FFI RustError mult_pippenger_inf(void* out, const void* points, size_t npoints,
                                        const void* scalars, size_t ffi_affine_sz)
{   return one_shot(out, points, npoints, scalars, false, ffi_affine_sz);   }

SPPARK_FFI RustError mult_pippenger(void* out, const void* points, size_t npoints, const void* scalars)
{   return one_shot(out, points, npoints, scalars, false, 2 * sizeof(fp_d));   }

#ifndef SPPARK_NO_G2
// which accumulation kernel the G2 entry point runs (process-wide: its contexts are pooled): 0 = automatic (wave pairs,
// one Fp2 component per wave, for the 14-limb base fields; one lane per addition otherwise), 1 = wave pairs, 2 = one lane.
// Both compute the same buckets; the switch exists so that the tests hold BOTH against the oracle.
static std::atomic<unsigned> g2_path{0};
SPPARK_FFI RustError sppark_msm_g2_path(unsigned mode)
{   return guarded([&] { if (mode > 2) HIP_OK(hipErrorInvalidValue); g2_path.store(mode, std::memory_order_relaxed); });   }
// poc/msm-cuda/cuda/pippenger_inf.cu:41-47: the same over G2 (coordinates in Fp2)
SPPARK_FFI RustError mult_pippenger_fp2_inf(void* out, const void* points, size_t npoints,
                                            const void* scalars, size_t ffi_affine_sz)
{
    memset(out, 0, sizeof(point2_t));
    return guarded([&] {
        borrowed<msm2_impl> msm(-1);
        msm->tune.g2_coop = g2_path.load(std::memory_order_relaxed);
#ifdef SPPARK_TUNING
        // tuning builds: the plan knobs of the pooled G2 context (tools/gpu_g2_bench.py sweeps them)
        {
            struct g2k { const char* name; unsigned msm_tunables::*f; };
            static const g2k ks[] = {{"SPPARK_G2_WBITS", &msm_tunables::wbits}, {"SPPARK_G2_L", &msm_tunables::L}, {"SPPARK_G2_F", &msm_tunables::F},
                                     {"SPPARK_G2_K", &msm_tunables::K}, {"SPPARK_G2_K1", &msm_tunables::K1}, {"SPPARK_G2_TOP", &msm_tunables::top}
                                    };
            for (const g2k& k : ks) { const char* e = getenv(k.name); msm->tune.*(k.f) = e ? (unsigned)atoi(e) : 0u; }    // (pooled context: absent = automatic again)
            const char* e = getenv("SPPARK_G2_JOIN");       // the numeric code of sppark_msm_tune_tail
            if (!decode_tail_code(e ? (unsigned)atoi(e) : 0u, msm->tune.sw)) HIP_OK(hipErrorInvalidValue);
        }
#endif
        if (is_device_pointer(points) || is_device_pointer(scalars)) HIP_OK(hipDeviceSynchronize());
        point2_t r;
        msm->invoke(r, points, npoints, scalars, false, ffi_affine_sz);
        memcpy(out, &r, sizeof(r));
    });
}

#endif

// free the scratch memory kept by the idle one-shot contexts (all devices)
SPPARK_FFI void sppark_msm_release_cached(void)
{
    ctx_pool<msm_impl>::get().release_idle();
#ifndef SPPARK_NO_G2
    ctx_pool<msm2_impl>::get().release_idle();
#endif
    dev_scratch_pool::instance().release();     // the staging buffers of this library's NTT / LDE / polynomial entry points
}

// msm/batch_addition.cuh:25-132 (batch_addition / batch_diff, the bitmap variants; C++ templates in
// the reference): out = sum of the points whose bit is set in |bitmap|; with |refmap| the points of
// the symmetric difference, those only in |refmap| subtracted.  Maps: ceil(npoints/32) words, bit k
// of word w = point 32*w + k.  points / maps: host or device pointers.
SPPARK_FFI RustError sppark_batch_addition(void* out, const void* points, size_t npoints,
                                           const uint32_t* bitmap, const uint32_t* refmap, size_t ffi_affine_sz)
{
    store_inf(out);
    return guarded([&] {
        borrowed<msm_impl> msm(-1);
        if (is_device_pointer(points) || is_device_pointer(bitmap) || is_device_pointer(refmap)) HIP_OK(hipDeviceSynchronize());
        point_t r;
        msm->batch_add(r, points, npoints, bitmap, refmap, ffi_affine_sz);
        store_point(out, r);
    });
}

// number of usable devices (the filtered list of util/all_gpus.cpp:39-54; ngpus(), :62-63)
SPPARK_FFI size_t sppark_ngpus(void) { return gpus_t::all().size(); }

// Multi-GPU G1 MSM in one process: the vector is cut into ndev contiguous shards (shard i =
// [i*n/ndev, (i+1)*n/ndev)) that run concurrently on devices 0..ndev-1; ndev == 0 = all devices.
// points / scalars: HOST pointers (each device copies its own shard, chunk by chunk).
static RustError msm_multi_impl(void* out, const void* points, size_t npoints, const void* scalars,
                                int mont, size_t ffi_affine_sz, unsigned ndev, float* out_ms)
{
    store_inf(out);
    return guarded([&] {
        const size_t avail = gpus_t::all().size();
        if (avail == 0) HIP_OK(hipErrorNoDevice);
        if (ndev == 0) ndev = (unsigned)avail;
        if (ndev > avail || ffi_affine_sz < 2 * sizeof(fp_h) || (npoints && (!points || !scalars))) HIP_OK(hipErrorInvalidValue);
        std::vector<const void*> p(ndev), s(ndev);
        std::vector<size_t> n(ndev);
        std::vector<int> ids(ndev);
        const size_t base = npoints / ndev, rem = npoints % ndev;
        for (unsigned i = 0; i < ndev; i++) {
            size_t lo = i * base + std::min<size_t>(i, rem);
            n[i] = base + (i < rem ? 1 : 0);
            p[i] = (const char*)points + lo * ffi_affine_sz;
            s[i] = (const char*)scalars + lo * sizeof(fr_d);
            ids[i] = (int)i;
        }
        point_t r;
        msm_shards(r, p.data(), n.data(), s.data(), mont != 0, ffi_affine_sz, ndev, ids.data(), out_ms);
        store_point(out, r);
    });
}
SPPARK_FFI RustError sppark_msm_multi(void* out, const void* points, size_t npoints, const void* scalars,
                                      int mont, size_t ffi_affine_sz, unsigned ndev)
{   return msm_multi_impl(out, points, npoints, scalars, mont, ffi_affine_sz, ndev, nullptr);   }
// the same, and out_ms[i] = wall-clock milliseconds device i spent on its shard (ndev entries; with ndev == 0
// the caller provides sppark_ngpus() entries)
SPPARK_FFI RustError sppark_msm_multi_ms(void* out, const void* points, size_t npoints, const void* scalars,
                                         int mont, size_t ffi_affine_sz, unsigned ndev, float* out_ms)
{   return msm_multi_impl(out, points, npoints, scalars, mont, ffi_affine_sz, ndev, out_ms);   }
// The general form: nshards independent (points, npoints, scalars) triples, shard i on device
// device_ids[i] (index in the filtered list; NULL = device i).  Pointers may be host pointers or
// pointers into the memory of the shard's own device.  A device may appear more than once.
static RustError msm_multi_shards_impl(void* out, const void* const* points, const size_t* npoints,
                                       const void* const* scalars, int mont, size_t ffi_affine_sz,
                                       unsigned nshards, const int* device_ids, float* out_ms)
{
    store_inf(out);
    return guarded([&] {
        if (nshards && (!points || !npoints || !scalars)) HIP_OK(hipErrorInvalidValue);
        if (ffi_affine_sz < 2 * sizeof(fp_h)) HIP_OK(hipErrorInvalidValue);
        const size_t avail = gpus_t::all().size();
        for (unsigned i = 0; i < nshards; i++) {
            int id = device_ids ? device_ids[i] : (int)i;
            if (id < 0 || (size_t)id >= avail) HIP_OK(hipErrorInvalidDevice);
        }
        point_t r;
        msm_shards(r, points, npoints, scalars, mont != 0, ffi_affine_sz, nshards, device_ids, out_ms);
        store_point(out, r);
    });
}
SPPARK_FFI RustError sppark_msm_multi_shards(void* out, const void* const* points, const size_t* npoints,
                                             const void* const* scalars, int mont, size_t ffi_affine_sz,
                                             unsigned nshards, const int* device_ids)
{   return msm_multi_shards_impl(out, points, npoints, scalars, mont, ffi_affine_sz, nshards, device_ids, nullptr);   }
SPPARK_FFI RustError sppark_msm_multi_shards_ms(void* out, const void* const* points, const size_t* npoints,
                                                const void* const* scalars, int mont, size_t ffi_affine_sz,
                                                unsigned nshards, const int* device_ids, float* out_ms)
{   return msm_multi_shards_impl(out, points, npoints, scalars, mont, ffi_affine_sz, nshards, device_ids, out_ms);   }

// ---- one PROCESS per GPU: the exchange step over the caller's RCCL communicator ------------------------------
// (north star: "RCCL exchange"; the reference has no multi-GPU MSM -- one gpu_t per msm_t, msm/pippenger.cuh:328-353.)
// Elliptic-curve addition is not an RCCL reduction operator, so the exchange is ONE ncclAllGather of the ranks'
// Jacobian partial sums (144 bytes each for BLS12-381 G1) and every rank adds the nranks points on its host:
// all ranks return the same point.  RCCL is bound at run time (util/rccl_dyn.hpp).
// |out| may be the same buffer as |partial| (the natural call after an MSM entry point wrote |out|): the partial sum is
// copied before |out| is cleared.
SPPARK_FFI RustError sppark_msm_rccl_sum(void* out, const void* partial, int g2, void* nccl_comm, void* stream)
{
#ifndef SPPARK_NO_G2
    const size_t bytes = g2 ? sizeof(point2_t) : sizeof(point_t);
    unsigned char mine[sizeof(point2_t)];
    if (partial) memcpy(mine, partial, bytes);
    memset(out, 0, bytes);
    return guarded([&] {
        const void* src = partial ? mine : nullptr;
        if (g2) rccl_sum<point2_t>(out, src, nccl_comm, stream); else rccl_sum<point_t>(out, src, nccl_comm, stream);
    });
#else
    unsigned char mine[sizeof(point_t)];
    if (partial) memcpy(mine, partial, sizeof(point_t));
    store_inf(out);
    return guarded([&] {
        if (g2) throw hip_error(ENOTSUP, "this curve has no G2");
        rccl_sum<point_t>(out, partial ? mine : nullptr, nccl_comm, stream);
    });
#endif
}
// A rank's whole share of a sharded G1 MSM: the local MSM over its shard (the arguments of mult_pippenger_inf, plus
// |mont|) on the calling thread's current device, then the exchange.  Collective: every rank of |nccl_comm| calls it
// (a rank without points passes npoints == 0).
SPPARK_FFI RustError sppark_msm_rccl(void* out, const void* points, size_t npoints, const void* scalars,
                                     int mont, size_t ffi_affine_sz, void* nccl_comm, void* stream)
{
    unsigned char part[sizeof(point_t)];
    RustError e = one_shot(part, points, npoints, scalars, mont != 0, ffi_affine_sz);
    // (a rank that failed locally still takes part in the collective with the point at infinity one_shot() left: the
    // others must not hang in it; this rank reports its own error)
    RustError x = sppark_msm_rccl_sum(out, part, 0, nccl_comm, stream);
    if (e.code) { free(x.message); store_inf(out); return e; }
    return x;
}

SPPARK_FFI RustError sppark_msm_create(sppark_msm_ctx** ctx, int device_id, void* stream)
{
    *ctx = nullptr;
    return guarded([&] { *ctx = new sppark_msm_ctx(device_id, (hipStream_t)stream); });
}
SPPARK_FFI void sppark_msm_destroy(sppark_msm_ctx* ctx) { delete ctx; }
SPPARK_FFI RustError sppark_msm_set_stream(sppark_msm_ctx* ctx, void* stream)
{   return guarded([&] { ctx->impl.set_stream((hipStream_t)stream); });   }
SPPARK_FFI RustError sppark_msm_tune(sppark_msm_ctx* ctx, unsigned wbits, unsigned L, unsigned F,
                                     unsigned K, unsigned nslabs)
{
    return guarded([&] {
        if ((K & (K - 1)) || wbits > 26) HIP_OK(hipErrorInvalidValue);     // (25, 26: fixed-base tables only; an ordinary plan stops at 24)
        ctx->impl.tune.wbits = wbits; ctx->impl.tune.L = L; ctx->impl.tune.F = F;
        ctx->impl.tune.K = K; ctx->impl.tune.nslabs = nslabs;
    });
}
// split of the bucket index between the two sort levels (0 = automatic)
SPPARK_FFI RustError sppark_msm_tune_sort(sppark_msm_ctx* ctx, unsigned low_bits)
{   return guarded([&] { ctx->impl.tune.LB = low_bits; });   }
// level-A partitions with more entries than this are sorted by several work-groups (0 = 2^18)
SPPARK_FFI RustError sppark_msm_tune_split(sppark_msm_ctx* ctx, unsigned big_partition)
{   return guarded([&] { ctx->impl.tune.big = big_partition; });   }
// bucket sums: windows with at most this many partial sums go to the subset-sum top (0 = automatic, 1 = never)
SPPARK_FFI RustError sppark_msm_tune_sums(sppark_msm_ctx* ctx, unsigned top_items)
{   return guarded([&] { ctx->impl.tune.top = top_items; });   }
// the tail of an MSM: join = the numeric code of an A/B switch (the table at msm_plan.hpp decode_tail_code; 0 = none);
// k1 = buckets per work item of the first bucket-sum level (a power of two; 0 = as the other levels)
SPPARK_FFI RustError sppark_msm_tune_tail(sppark_msm_ctx* ctx, unsigned join, unsigned k1)
{
    return guarded([&] {
        msm_switches sw;
        if ((k1 & (k1 - 1)) || !decode_tail_code(join, sw)) HIP_OK(hipErrorInvalidValue);
        ctx->impl.tune.sw = sw; ctx->impl.tune.K1 = k1;
    });
}
// pipeline shape: window groups (0 = automatic, 1 = single stream), points per chunk of the
// chunked path (0 = automatic), upper bound of the scratch memory in bytes (0 = what the device has)
SPPARK_FFI RustError sppark_msm_tune_pipeline(sppark_msm_ctx* ctx, unsigned groups, size_t chunk_points, size_t max_scratch_bytes)
{   return guarded([&] { ctx->impl.tune.groups = groups; ctx->impl.tune.chunk = chunk_points; ctx->impl.tune.max_scratch = max_scratch_bytes; });   }
SPPARK_FFI unsigned sppark_msm_last_chunks(const sppark_msm_ctx* ctx) { return ctx->impl.chunks_of_last_invoke(); }
SPPARK_FFI unsigned sppark_msm_tail_redone(const sppark_msm_ctx* ctx) { return ctx->impl.tail_redone(); }
SPPARK_FFI RustError sppark_msm_reserve(sppark_msm_ctx* ctx, size_t npoints, size_t ffi_affine_sz,
                                        int host_points, int host_scalars)
{   return guarded([&] { ctx->impl.reserve_for(npoints, ffi_affine_sz, host_points, host_scalars); });   }
SPPARK_FFI RustError sppark_msm_invoke(sppark_msm_ctx* ctx, void* out, const void* points, size_t npoints,
                                       const void* scalars, int mont, size_t ffi_affine_sz)
{
    store_inf(out);
    return guarded([&] {
        point_t r;
        ctx->impl.invoke(r, points, npoints, scalars, mont != 0, ffi_affine_sz);
        store_point(out, r);
    });
}
SPPARK_FFI RustError sppark_msm_set_points(sppark_msm_ctx* ctx, const void* points, size_t npoints, size_t ffi_affine_sz)
{   return guarded([&] { ctx->impl.preload(points, npoints, ffi_affine_sz); });   }
// the same, and the fixed-base tables of the points are built too (G1 fields with their own bucket records): later
// sppark_msm_invoke(ctx, out, NULL, npoints, ...) calls over exactly these npoints points run as ONE window over
// windows x npoints (digit, multiple) pairs; windows x the memory of the plain copy
SPPARK_FFI RustError sppark_msm_set_points_fixed_base(sppark_msm_ctx* ctx, const void* points, size_t npoints, size_t ffi_affine_sz)
{   return guarded([&] { ctx->impl.preload(points, npoints, ffi_affine_sz, true); });   }
SPPARK_FFI unsigned sppark_msm_fixed_base_windows(const sppark_msm_ctx* ctx) { return ctx->impl.fixed_base_windows(); }
SPPARK_FFI size_t sppark_msm_preloaded(const sppark_msm_ctx* ctx) { return ctx->impl.preloaded(); }
SPPARK_FFI RustError sppark_msm_enable_timing(sppark_msm_ctx* ctx, int on)
{   return guarded([&] { ctx->impl.enable_timing(on != 0); });   }
SPPARK_FFI float sppark_msm_kernel_ms(const sppark_msm_ctx* ctx, int which) { return ctx->impl.kernel_ms(which); }
SPPARK_FFI size_t sppark_msm_scratch_bytes(const sppark_msm_ctx* ctx) { return ctx->impl.scratch_bytes(); }
// plan the context would use for |npoints|: out = {window bits (longest), windows, buckets per window,
// run length L, level-A partitions, level-B low bits, record fan-in F, bucket chunk K}
SPPARK_FFI void sppark_msm_plan(const sppark_msm_ctx* ctx, size_t npoints, unsigned out[8])
{
    msm_plan p = ctx->impl.plan_for(npoints);
    out[0] = p.wbits; out[1] = p.nwins; out[2] = p.NB; out[3] = p.L; out[4] = p.NA; out[5] = p.LB; out[6] = p.F; out[7] = p.K;
}
// the sort's side of the plan: out = { slabs, points per slab, index bits kept in a 4-byte level-A record (0: 8-byte records),
// log2 slabs per index group, index groups, window groups, first-level bucket chunk, pieces per bucket the piece tree takes }
SPPARK_FFI void sppark_msm_plan_sort(const sppark_msm_ctx* ctx, size_t npoints, unsigned out[8])
{
    msm_plan p = ctx->impl.plan_for(npoints);
    out[0] = p.nslabs; out[1] = p.slab_sz; out[2] = p.IB; out[3] = p.SH; out[4] = p.NG; out[5] = p.G; out[6] = p.K1;
    out[7] = ctx->impl.piece_tree_cmax(p);
}
// ---- short scalars (include/sppark_amd_short.h): the caller declares the bit length, only its windows run -------
// (the contract is checked first -- msm_t::check_short --: a refused call selects no device and reads nothing)
SPPARK_FFI RustError sppark_msm_invoke_bits(sppark_msm_ctx* ctx, void* out, const void* points, size_t npoints,
                                            const void* scalars, unsigned scalar_bits, size_t scalar_stride, size_t ffi_affine_sz)
{
    store_inf(out);
    return guarded([&] {
        point_t r;
        ctx->impl.invoke_short(r, points, npoints, scalars, scalar_bits, scalar_stride, ffi_affine_sz);
        store_point(out, r);
    });
}
SPPARK_FFI RustError sppark_msm_reserve_bits(sppark_msm_ctx* ctx, size_t npoints, size_t ffi_affine_sz, int host_points, int host_scalars,
                                             unsigned scalar_bits, size_t scalar_stride)
{
    return guarded([&] {
        msm_impl::check_short(scalar_bits, scalar_stride, nullptr);
        ctx->impl.reserve_for(npoints, ffi_affine_sz, host_points, host_scalars, msm_impl::scalar_form(scalar_bits, scalar_stride));
    });
}
SPPARK_FFI void sppark_msm_plan_bits(const sppark_msm_ctx* ctx, size_t npoints, unsigned scalar_bits, unsigned out[8])
{
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (scalar_bits == 0 || scalar_bits > msm_impl::SHORT_BITS_MAX) return;
    msm_plan p = ctx->impl.plan_for(npoints, scalar_bits);
    out[0] = p.wbits; out[1] = p.nwins; out[2] = p.NB; out[3] = p.L; out[4] = p.NA; out[5] = p.LB; out[6] = p.F; out[7] = p.K;
}
SPPARK_FFI RustError mult_pippenger_inf_bits(void* out, const void* points, size_t npoints, const void* scalars,
                                             unsigned scalar_bits, size_t scalar_stride, size_t ffi_affine_sz)
{
    store_inf(out);
    return guarded([&] {
        msm_impl::check_short(scalar_bits, scalar_stride, scalars);
        borrowed<msm_impl> msm(-1);
        if (is_device_pointer(points) || is_device_pointer(scalars)) HIP_OK(hipDeviceSynchronize());     // (as one_shot())
        point_t r;
        msm->invoke_short(r, points, npoints, scalars, scalar_bits, scalar_stride, ffi_affine_sz);
        store_point(out, r);
    });
}
#ifndef SPPARK_NO_G2
SPPARK_FFI RustError mult_pippenger_fp2_inf_bits(void* out, const void* points, size_t npoints, const void* scalars,
                                                 unsigned scalar_bits, size_t scalar_stride, size_t ffi_affine_sz)
{
    memset(out, 0, sizeof(point2_t));
    return guarded([&] {
        msm2_impl::check_short(scalar_bits, scalar_stride, scalars);
        borrowed<msm2_impl> msm(-1);
        msm->tune.g2_coop = g2_path.load(std::memory_order_relaxed);
        if (is_device_pointer(points) || is_device_pointer(scalars)) HIP_OK(hipDeviceSynchronize());
        point2_t r;
        msm->invoke_short(r, points, npoints, scalars, scalar_bits, scalar_stride, ffi_affine_sz);
        memcpy(out, &r, sizeof(r));
    });
}
#endif

SPPARK_FFI RustError sppark_msm_tune_records(sppark_msm_ctx* ctx, unsigned records)
{   return guarded([&] { if (records > 2) throw hip_error(-(int)hipErrorInvalidValue, "tune_records"); ctx->impl.tune.records = records; });   }
// window groups the context would use for |npoints|
SPPARK_FFI unsigned sppark_msm_plan_groups(const sppark_msm_ctx* ctx, size_t npoints) { return ctx->impl.plan_for(npoints).G; }

// ---- host-side point helpers (no GPU work) --------------------------------
SPPARK_FFI void sppark_g1_jacobian_sum(void* out, const void* points, size_t n)
{
    point_t acc; acc.set_inf();
    for (size_t i = 0; i < n; i++) {
        point_t p; memcpy(&p, (const char*)points + i * sizeof(point_t), sizeof(p));
        acc.add(p);
    }
    store_point(out, acc);
}
SPPARK_FFI void sppark_g1_to_affine(void* out_xy, const void* jacobian)
{
    point_t p; memcpy(&p, jacobian, sizeof(p));
    fp_h xy[2];
    p.to_affine(xy[0], xy[1]);
    memcpy(out_xy, xy, sizeof(xy));
}

#ifndef SPPARK_NO_G2
// G2 twins of the host helpers
SPPARK_FFI void sppark_g2_jacobian_sum(void* out, const void* points, size_t n)
{
    point2_t acc; acc.set_inf();
    for (size_t i = 0; i < n; i++) {
        point2_t p; memcpy(&p, (const char*)points + i * sizeof(point2_t), sizeof(p));
        acc.add(p);
    }
    memcpy(out, &acc, sizeof(acc));
}
SPPARK_FFI void sppark_g2_to_affine(void* out_xy, const void* jacobian)
{
    point2_t p; memcpy(&p, jacobian, sizeof(p));
    fp2_h xy[2];
    p.to_affine(xy[0], xy[1]);
    memcpy(out_xy, xy, sizeof(xy));
}

#endif

} // extern "C"

// ---- synthetic-input generator: P_i = k_i * G on the device ------------------
__device__ __forceinline__ u64 splitmix64_at(u64 seed, u64 j)
{
    u64 z = seed + (j + 1) * 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(64)
void k_generate(wire_bucket_m* out, unsigned n, u64 seed)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    affine_dev<fp_d> g;
    u32 gx[fp_d::N], gy[fp_d::N];
    #pragma unroll
    for (int k = 0; k < fp_d::N / 2; k++) {
        gx[2*k] = (u32)curve_p::GX64[k]; gx[2*k+1] = (u32)(curve_p::GX64[k] >> 32);
        gy[2*k] = (u32)curve_p::GY64[k]; gy[2*k+1] = (u32)(curve_p::GY64[k] >> 32);
    }
    g.X = fp_d::from_wire(gx); g.Y = fp_d::from_wire(gy);
    g.inf = false;
    u64 kw[4];
    for (int w = 0; w < 4; w++) kw[w] = splitmix64_at(seed, (u64)i * 4 + w);
    kw[3] &= 0x1fffffffffffffffULL;                     // 253-bit
    xyzz_dev<fp_d> acc; acc.set_inf();
    for (int w = 3; w >= 0; w--) {
        u64 word = kw[w];
        for (int b = 63; b >= 0; b--) {
            acc.dbl();
            if ((word >> b) & 1) acc.madd(g, false);
        }
    }
    acc.store(&out[i]);
}

SPPARK_FFI RustError sppark_g1_generate(void* out, size_t stride, size_t n, uint64_t seed)
{
    return guarded([&] {
        if (n == 0) return;
        (void)select_gpu(-1);
        typedef wire_bucket_m bucket_t;
        bucket_t* d_pts;
        HIP_OK(hipMalloc((void**)&d_pts, n * sizeof(bucket_t)));
        hipLaunchKernelGGL(k_generate, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d_pts, (unsigned)n, seed);
        std::vector<fp_h> c(4 * n);
        hipError_t e = hipMemcpy(c.data(), d_pts, n * sizeof(bucket_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_pts);
        HIP_OK(e);
        // x = X/ZZ, y = Y/ZZZ with one shared inversion (Montgomery's trick)
        std::vector<fp_h> pref(2 * n + 1);
        pref[0] = fp_h::one();
        for (size_t i = 0; i < n; i++) {
            fp_h zzz = c[4*i+2], zz = c[4*i+3];
            if (zzz.is_zero()) zzz = fp_h::one();
            if (zz.is_zero())  zz  = fp_h::one();
            pref[2*i+1] = pref[2*i] * zz;
            pref[2*i+2] = pref[2*i+1] * zzz;
        }
        fp_h inv = pref[2*n].inverse();
        const size_t fb = sizeof(fp_h);
        std::vector<unsigned char> host(n * stride, 0);
        for (size_t i = n; i--;) {
            fp_h zzz = c[4*i+2], zz = c[4*i+3];
            bool is_inf = zzz.is_zero() && zz.is_zero();
            if (zzz.is_zero()) zzz = fp_h::one();
            if (zz.is_zero())  zz  = fp_h::one();
            fp_h izzz = inv * pref[2*i+1]; inv = inv * zzz;
            fp_h izz  = inv * pref[2*i];   inv = inv * zz;
            if (!is_inf) {
                fp_h x = c[4*i] * izz, y = c[4*i+1] * izzz;
                memcpy(&host[i * stride], &x, fb);
                memcpy(&host[i * stride + fb], &y, fb);
            } else if (stride > 2 * fb) {
                host[i * stride + 2 * fb] = 1;
            }
        }
        if (is_device_pointer(out)) HIP_OK(hipMemcpy(out, host.data(), host.size(), hipMemcpyHostToDevice));
        else                        memcpy(out, host.data(), host.size());
    });
}

// ---- all-distinct synthetic inputs: P_i = (a + i*b) * G, affine, written on the device -------
// The reference's own MSM test holds the result against an oracle on ARBITRARY points
// (poc/msm-cuda/tests/msm.rs:19-39); at 2^26 points no CPU oracle finishes, but a vector whose discrete
// logarithms are known needs none: sum s_i P_i = (sum s_i (a + i b) mod r) * G.  T lanes; lane t walks
// i = t, t + T, t + 2T, ... by mixed additions of the affine step (T b) G, so that the lanes of a wave
// touch adjacent points; the XYZZ chain is normalised by ONE inversion per lane (Montgomery's trick
// over the lane's ZZ * ZZZ), second walk backwards.  a >= 1 and a + n b < 2^127 < r: no point at infinity.
struct prog_par { u64 a_lo, a_hi, b_lo, b_hi; };

__device__ __forceinline__ fp_d fp_inverse(const fp_d& x)
{                                                       // x^(p-2), left to right
    u32 e[fp_d::N];
    u32 bw = 2;
    #pragma unroll
    for (int i = 0; i < fp_d::N; i++) {
        u32 m = (u32)curve_p::fp::MOD[i];
        e[i] = m - bw; bw = m < bw ? 1u : 0u;
    }
    fp_d r = fp_d::one();
    for (int i = fp_d::N - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = r.sqr();
            if ((e[i] >> b) & 1) r = r * x;
        }
    return r;
}

__device__ __forceinline__ void g1_mul_u128(wire_bucket_d& acc, const affine_dev<fp_d>& g, u64 lo, u64 hi)
{
    acc.set_inf();
    for (int w = 1; w >= 0; w--) {
        u64 word = w ? hi : lo;
        for (int b = 63; b >= 0; b--) {
            acc.dbl();
            if ((word >> b) & 1) acc.madd(g, false);
        }
    }
}

__device__ __forceinline__ affine_dev<fp_d> g1_generator_dev()
{
    affine_dev<fp_d> g;
    u32 gx[fp_d::N], gy[fp_d::N];
    #pragma unroll
    for (int k = 0; k < fp_d::N / 2; k++) {
        gx[2*k] = (u32)curve_p::GX64[k]; gx[2*k+1] = (u32)(curve_p::GX64[k] >> 32);
        gy[2*k] = (u32)curve_p::GY64[k]; gy[2*k+1] = (u32)(curve_p::GY64[k] >> 32);
    }
    g.X = fp_d::from_wire(gx); g.Y = fp_d::from_wire(gy); g.inf = false;
    return g;
}

__device__ __forceinline__ void fp_store8(unsigned char* p, const fp_d& x)      // 8-byte aligned destinations (stride 104)
{
    u32 w[fp_d::N]; x.to_wire(w);
    uint2* d = reinterpret_cast<uint2*>(p);
    #pragma unroll
    for (int i = 0; i < fp_d::N / 2; i++) d[i] = make_uint2(w[2*i], w[2*i+1]);
}
__device__ __forceinline__ fp_d fp_load8(const unsigned char* p)
{
    u32 w[fp_d::N];
    const uint2* d = reinterpret_cast<const uint2*>(p);
    #pragma unroll
    for (int i = 0; i < fp_d::N / 2; i++) { uint2 v = d[i]; w[2*i] = v.x; w[2*i+1] = v.y; }
    return fp_d::from_wire(w);
}

// step = (T b) G as an affine point (one lane; 128 doublings and one inversion)
__global__ void k_progression_step(unsigned char* step_xy, u64 s_lo, u64 s_hi)
{
    if (threadIdx.x | blockIdx.x) return;
    wire_bucket_d acc;
    g1_mul_u128(acc, g1_generator_dev(), s_lo, s_hi);
    fp_d iz = fp_inverse(acc.ZZZ);                      // 1/ZZZ; 1/ZZ = ZZ^2 / ZZZ^2
    fp_d izz = (acc.ZZ * iz).sqr();
    fp_store8(step_xy, acc.X * izz);
    fp_store8(step_xy + sizeof(fp_d), acc.Y * iz);
}

__global__ __launch_bounds__(64)
void k_progression(unsigned char* out, unsigned stride, size_t n, unsigned T, prog_par par,
                   const unsigned char* step_xy, unsigned step_inf, unsigned char* tmp /* n x 3 field elements: ZZZ | ZZ | prefix */)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T || t >= n) return;
    constexpr size_t FB = sizeof(fp_d);
    affine_dev<fp_d> step; step.X = fp_load8(step_xy); step.Y = fp_load8(step_xy + FB); step.inf = step_inf != 0;
    // k_t = a + t b (128-bit)
    unsigned __int128 k = ((unsigned __int128)par.a_hi << 64 | par.a_lo) + ((unsigned __int128)par.b_hi << 64 | par.b_lo) * t;
    wire_bucket_d acc;
    g1_mul_u128(acc, g1_generator_dev(), (u64)k, (u64)(k >> 64));
    fp_d pref = fp_d::one();
    for (size_t i = t; i < n; i += T) {                 // forward: X | Y into the output slot, ZZZ | ZZ | prefix aside
        unsigned char* o = out + i * stride;
        unsigned char* s = tmp + i * 3 * FB;
        fp_store8(o, acc.X); fp_store8(o + FB, acc.Y);
        fp_store8(s, acc.ZZZ); fp_store8(s + FB, acc.ZZ); fp_store8(s + 2 * FB, pref);
        pref = pref * (acc.ZZZ * acc.ZZ);
        acc.madd(step, false);
    }
    fp_d inv = fp_inverse(pref);
    size_t cnt = (n - t + T - 1) / T;
    for (size_t j = cnt; j--;) {                        // backward
        size_t i = t + j * (size_t)T;
        unsigned char* o = out + i * stride;
        const unsigned char* s = tmp + i * 3 * FB;
        fp_d zzz = fp_load8(s), zz = fp_load8(s + FB), pre = fp_load8(s + 2 * FB);
        fp_d id = inv * pre;                            // 1 / (ZZZ ZZ) of point i
        inv = inv * (zzz * zz);
        fp_d x = fp_load8(o) * (zzz * id), y = fp_load8(o + FB) * (zz * id);
        fp_store8(o, x); fp_store8(o + FB, y);
        for (unsigned b = 2 * FB; b < stride; b++) o[b] = 0;     // Affine_inf_t: flag byte and padding clear
    }
}

SPPARK_FFI RustError sppark_g1_generate_progression(void* out, size_t stride, size_t n, const uint64_t a[2], const uint64_t b[2])
{
    return guarded([&] {
        if (n == 0) return;
        constexpr size_t FB = sizeof(fp_h);
        if (stride < 2 * FB || (stride & 7)) throw hip_error(-(int)hipErrorInvalidValue, "generate_progression: stride");
        if (!is_device_pointer(out)) throw hip_error(-(int)hipErrorInvalidValue, "generate_progression: out must be a device pointer");
        unsigned __int128 A = (unsigned __int128)a[1] << 64 | a[0], B = (unsigned __int128)b[1] << 64 | b[0];
        // a >= 1, a + n b < 2^127 (below every scalar-field modulus here): all k_i distinct and non-zero mod r
        if (A == 0 || (B >> 96) != 0 || (A >> 126) != 0 || (n >> 30) != 0) throw hip_error(-(int)hipErrorInvalidValue, "generate_progression: range");
        (void)select_gpu(-1);
        unsigned T = (unsigned)std::min<size_t>(n, (size_t)1 << 18);
        unsigned __int128 S = B * T;
        unsigned char *tmp, *step;
        HIP_OK(hipMalloc((void**)&tmp, n * 3 * FB));
        if (hipError_t e = hipMalloc((void**)&step, 2 * FB)) { (void)hipFree(tmp); HIP_OK(e); }
        (void)hipMemset(step, 0, 2 * FB);
        prog_par par = { a[0], a[1], b[0], b[1] };
        if (S != 0)
            hipLaunchKernelGGL(k_progression_step, dim3(1), dim3(64), 0, 0, step, (u64)S, (u64)(S >> 64));
        hipLaunchKernelGGL(k_progression, dim3((T + 63) / 64), dim3(64), 0, 0, (unsigned char*)out, (unsigned)stride, n, T, par, step, S == 0 ? 1u : 0u, tmp);
        hipError_t e = hipDeviceSynchronize();
        (void)hipFree(tmp); (void)hipFree(step);
        HIP_OK(e);
    });
}
