// Host driver of the MI355X MSM pipeline: plays the role of the reference's
// msm_t (msm/pippenger.cuh:325-728) -- window choice, device scratch, kernel
// sequence, error mapping -- re-planned for a 288 GB / 256-CU part:
//
//  * WINDOW GROUPS (a tunable, off by default).  The W windows can be cut into G groups that are
//    sorted and accumulated one after the other, the digits + counting sort of group g+1 on an
//    auxiliary stream (optionally confined to a few CUs, hipExtStreamCreateWithCUMask) beside the
//    bucket accumulation of group g on the main one; the record tree and the bucket sums still run
//    once, for all windows (their ~15 dependent launches are latency-bound).  Scratch for digits /
//    partitions / sorted lists is then two group-sized sets instead of W.  It does NOT make an MSM
//    faster on MI355X: the sort kernels were shrunk to fit beside k_accumulate on a CU (512 lanes,
//    16 VGPRs) and they do run concurrently, but the accumulation slows down by what the sort
//    gains -- measured for 1..12 groups, 4..256 CUs for the sort stream and three stream
//    priorities (profiles/r02_msm_groups.log).  (The reference overlaps its sort with the previous
//    batch's accumulation through a 3-stream flip-flop over POINT batches, pippenger.cuh:494-557.)
//  * CHUNKS.  Host-resident inputs (what mult_pippenger_inf's callers pass) are cut into
//    point chunks: chunk c+1 is copied to the device (scalars first) while chunk c is being
//    computed; every chunk is a complete MSM and the partial results are added on the host.
//    The same loop bounds the scratch memory: when the device cannot hold the scratch of the
//    whole MSM (or tune.max_scratch says so) the chunk is halved until it does, for host AND
//    device-resident inputs.  The reference streams 2^24-point strides for the same two
//    reasons (pippenger.cuh:454-459,494-557).
//  * no cooperative launches or device-global work counters (:157-223): kernel
//    boundaries are the only grid-wide synchronisation;
//  * the host part is O(windows): it receives one XYZZ sum per window and runs
//    the Horner recombination (the reference integrates 256 partial sums per
//    window on a host thread pool, :627-727).
//
// Inputs may be host or device pointers (cf. is_device_ptr, util/gpu_t.cuh:385-395,
// and the preloaded-points constructor :351-388).
#pragma once
#include "msm_kernels.hpp"
#include "msm_coop_kernels.hpp"
#include "msm_route.hpp"
#include "../ec/jacobian_host.hpp"
#include "../util/runtime.hpp"
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

namespace sppark_amd {

// FD: device coordinate field (fp_class<P> for G1, fp2_dev<P> for G2), FH: its host
// twin with the same memory image (mont_host<P> / fp2_host<P>), FRp: scalar field.
template<class FD, class FH, class FRp>
class msm_t {
public:
    typedef FD fp_d;
    // the coordinate field is Fp2 over the loosely-reduced field: the cooperative accumulation exists for it
    static constexpr bool G2_COOP_BUILT = field_is_internal<FD>::value && !field_is_montx<FD>::value;
    typedef mont_dev<FRp> fr_d;
    typedef FH fp_h;
    typedef typename xyzz_dev<fp_d>::mem_t bucket_t;       // memory image: wire format
    typedef jacobian_host<fp_h> point_t;
    static constexpr int STD_WORDS = sizeof(FH) / 4;        // 32-bit words of a coordinate in the reference's wire form
    static constexpr size_t FP_BYTES = sizeof(FH);
    static constexpr bool INTERNAL = field_is_internal<FD>::value;      // ff/montx_dev.hpp: own point/bucket records
    static constexpr bool MONTX = field_is_montx<FD>::value;            // ... over the base field (G1): low-latency kernels, fixed-base tables
    typedef xyzz_mem<STD_WORDS> std_bucket_t;
    static_assert(INTERNAL || sizeof(FH) == 4 * FD::N, "host and device coordinate fields must share the wire image");
    static constexpr size_t SCALAR_BYTES = sizeof(fr_d);
    static constexpr unsigned MAX_WINS = 128;
    // what the route (msm_route.hpp) must know of the coordinate field
    static msm_field field()
    {
        bool pairs_default = false;
        if constexpr (G2_COOP_BUILT) pairs_default = fp_d::NL >= 14;
        return msm_field{INTERNAL, MONTX, G2_COOP_BUILT, pairs_default, (unsigned)fp_d::N, (unsigned)sizeof(bucket_t), (unsigned)FP_BYTES,
                         FRp::MOD, (unsigned)FRp::N};
    }
    static constexpr size_t FIXED_BASE_MIN = (size_t)1 << 23;      // points from which set_points_fixed_base builds tables by itself

private:
    const gpu_info* gpu;
    hipStream_t stream;                 // main stream: the caller's, or a private one
    bool own_stream;
    hipStream_t aux = nullptr;          // sort of the next window group
    unsigned gseq = 0;                  // running window-group counter: parity selects the buffer set
    hipStream_t cpy = nullptr;          // host -> device copies of the next chunk
    hipEvent_t join_ev = nullptr;
    hipEvent_t ev_fork = nullptr, ev_sorted[2] = {nullptr, nullptr}, ev_accdone[2] = {nullptr, nullptr};
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_chunkdone[2] = {nullptr, nullptr};
    unsigned char* blob = nullptr;
    size_t blob_sz = 0;
    unsigned char* stage = nullptr;     // two staging sets for host-resident chunks
    size_t stage_sz = 0;
    std_bucket_t* h_sums = nullptr;     // pinned: window sums of every chunk in flight
    size_t h_sums_cap = 0;
    u32* h_flag = nullptr;              // pinned: "a bucket had more pieces than the piece tree takes" of the last MSM (enqueue)
    const u32* h_flag_cur = nullptr;    // where invoke() reads that flag: |h_flag|, or the word behind the window sums (the small sizes)
    u32* d_pflag = nullptr;             // the small sizes' flag on the device: zero between MSMs (the kernel that hands it over clears it)
    bool piece_pending = false;         // the last enqueue ran the piece tree and left the fan-in tree out
    std::vector<hipEvent_t> tev;        // timing events: [0] start, [1] end, [2+2g], [3+2g] around k_accumulate of group g
    unsigned char* pre_points = nullptr;    // points kept on the device by preload() (msm_t ctor with points, pippenger.cuh:351-385)
    size_t pre_n = 0, pre_stride = 0;
    unsigned pre_fb_wbits = 0, pre_fb_nwins = 0;    // fixed-base tables: window bits / windows they were built for (0: none)
    float last_ms[4] = {0, 0, 0, 0};    // [0] before the first accumulation, [1] accumulation kernels, [2] whole device part, [3] accumulate launches
    unsigned last_chunks = 0;
    unsigned last_redo = 0;             // invocations whose tail ran twice (the piece tree met a bucket beyond its limit)
    bool timing = false;

    struct layout {
        size_t digits[2], sorted[2], partA[2], H[2], tot[2], offA[2], off[2], curB[2], bigl[2];
        size_t buckets, keyA, ptA, keyB, ptB, keyC, flag, A1, W1, A2, W2, conv, sums, total;
    };

    static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
    static constexpr size_t conv_stride()
    {
        if constexpr (INTERNAL) return affine_loader<FD>::STRIDE; else return 0;
    }

    layout make_layout(const msm_plan& p, bool convert) const
    {
        layout l; size_t o = 0;
        auto take = [&](size_t sz) { size_t r = o; o += align_up(sz); return r; };
        const size_t wg = p.wpg;
        for (unsigned b = 0; b < 2; b++) {
            if (b == 1 && p.G == 1) {               // a single group needs one set
                l.digits[1] = l.digits[0]; l.sorted[1] = l.sorted[0]; l.partA[1] = l.partA[0]; l.H[1] = l.H[0]; l.tot[1] = l.tot[0];
                l.offA[1] = l.offA[0]; l.off[1] = l.off[0]; l.curB[1] = l.curB[0]; l.bigl[1] = l.bigl[0];
                break;
            }
            l.digits[b] = take(wg * p.n * 4);
            l.sorted[b] = take(wg * p.n * 4);
            l.partA[b]  = take(wg * p.n * (p.IB ? 4 : 8));                         // level-A records: packed / wide
            l.H[b]      = take(wg * p.nslabs * p.NA * 4);
            l.tot[b]    = take(wg * p.NA * 4);
            l.offA[b]   = take(wg * (p.NA + 1) * 4);
            l.off[b]    = take(wg * ((size_t)p.NB + 1) * 4);
            l.curB[b]   = take(wg * ((size_t)p.NB + 1) * 4);                    // cursors of the cooperative sort
            l.bigl[b]   = take((wg * p.NA + 1) * 4);                            // [count | list of oversized partitions]
        }
        // buckets, records and bucket-sum levels: all windows (one record tree / bucket-sum chain per MSM)
        l.buckets = take((size_t)p.nwins * p.NB * sizeof(bucket_t));
        size_t nrecA = (size_t)2 * p.nwins * p.chunks_per_win;
        size_t nrecB = 2 * ((nrecA + p.F - 1) / p.F);
        l.keyA = take(nrecA * 4); l.ptA = take(nrecA * sizeof(bucket_t));
        l.keyB = take(nrecB * 4); l.ptB = take(nrecB * sizeof(bucket_t));
        l.keyC = take(nrecA * 4); l.flag = take(4);                 // k_join_runs: filtered keys, "a long segment exists"
        size_t n1 = (size_t)p.nwins * std::max<size_t>(p.NB / p.K1, lg2_floor(p.NB) + 1);      // (the small windows' m + 1 parts: k_bucket_small_bits_coop)
        l.A1 = take(n1 * sizeof(bucket_t)); l.W1 = take(n1 * sizeof(bucket_t));
        l.A2 = take(n1 * sizeof(bucket_t)); l.W2 = take(n1 * sizeof(bucket_t));
        l.conv = take(INTERNAL && convert ? (size_t)p.n * conv_stride() : 0);     // points in the field's own records
        l.sums = take(((size_t)p.nwins + 1) * std::max(sizeof(std_bucket_t), sizeof(bucket_t)));     // (+ the small sizes' flag word)
        l.total = o;
        return l;
    }

    void reserve(size_t sz)
    {
        if (sz <= blob_sz) return;
        if (blob) {
            HIP_OK(hipStreamSynchronize(stream));
            if (aux) HIP_OK(hipStreamSynchronize(aux));
            HIP_OK(hipFree(blob)); blob = nullptr; blob_sz = 0;
        }
        HIP_OK(dev_scratch_pool::malloc_or_drain((void**)&blob, sz));      // (idle staging buffers of this library go first)
        blob_sz = sz;
    }
    void reserve_stage(size_t sz)
    {
        if (sz <= stage_sz) return;
        if (stage) { HIP_OK(hipDeviceSynchronize()); HIP_OK(hipFree(stage)); stage = nullptr; stage_sz = 0; }
        HIP_OK(dev_scratch_pool::malloc_or_drain((void**)&stage, sz));
        stage_sz = sz;
    }
    void reserve_sums(size_t count)
    {
        if (count <= h_sums_cap) return;
        if (h_sums) { HIP_OK(hipStreamSynchronize(stream)); HIP_OK(hipHostFree(h_sums)); h_sums = nullptr; h_sums_cap = 0; }
        HIP_OK(hipHostMalloc((void**)&h_sums, count * sizeof(std_bucket_t), hipHostMallocDefault));
        h_sums_cap = count;
    }
    void need_event(hipEvent_t& e) { if (!e) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    // hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, raised at most once per (context, kernel, size step):
    // the call costs a few microseconds of host time on every launch path otherwise
    // (the record lives in the CONTEXT: a process-wide one would be stale after a hipDeviceReset, and the next launch
    // with more than 64 KB of dynamic LDS would fail; a context does not outlive its device)
    std::map<const void*, size_t> lds_done;
    void lds_attr(const void* fn, size_t bytes)
    {
        size_t& have = lds_done[fn];
        if (bytes <= have) return;
        HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        have = bytes;
    }
    void need_aux()
    {
        if (aux) return;
        // The sort of the following window groups: an ordinary stream on all CUs.  (Tuning builds, -DSPPARK_TUNING:
        // SPPARK_MSM_AUX_CUS=N confines it to N compute units.)
        unsigned ncu = 0;
#ifdef SPPARK_TUNING
        if (const char* e = getenv("SPPARK_MSM_AUX_CUS")) ncu = (unsigned)atoi(e);
#endif
        const unsigned total = (unsigned)gpu->prop.multiProcessorCount;
        hipError_t err = hipErrorNotSupported;
        if (ncu && ncu < total) {
            std::vector<uint32_t> mask((total + 31) / 32, 0);
            for (unsigned k = 0; k < ncu; k++) {        // spread over the whole CU index range (all XCDs / shader engines)
                unsigned cu = (unsigned)(((uint64_t)k * total) / ncu);
                mask[cu / 32] |= 1u << (cu % 32);
            }
            err = hipExtStreamCreateWithCUMask(&aux, (uint32_t)mask.size(), mask.data());
            if (err != hipSuccess) { (void)hipGetLastError(); aux = nullptr; }
        }
        if (!aux) HIP_OK(hipStreamCreateWithFlags(&aux, hipStreamNonBlocking));
        need_event(ev_fork);
        for (int b = 0; b < 2; b++) { need_event(ev_sorted[b]); need_event(ev_accdone[b]); }
    }
    void need_cpy()
    {
        if (cpy) return;
        HIP_OK(hipStreamCreateWithFlags(&cpy, hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) { need_event(ev_copied[b]); need_event(ev_chunkdone[b]); }
    }
    void need_tev(size_t count)
    {
        while (tev.size() < count) { hipEvent_t e; HIP_OK(hipEventCreate(&e)); tev.push_back(e); }
    }

public:
    msm_tunables tune;

    explicit msm_t(int device_id = -1, hipStream_t s = nullptr)
        : gpu(&select_gpu(device_id)), stream(s), own_stream(false)
    {
        {
            // lanes of k_accumulate the device runs at once -- at most two waves per SIMD (two 256-lane work-groups per CU):
            // a third resident wave adds no throughput -- : the plan fits the accumulation's grid to whole rounds of them
            // (asked on the context's OWN device, not whichever one happens to be current: the answer feeds the plan)
            int nb = 0, cur = -1;
            (void)hipGetDevice(&cur);
            if (cur != gpu->hip_id) HIP_OK(hipSetDevice(gpu->hip_id));
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_accumulate<fp_d, false>, 256, 0) == hipSuccess && nb > 0)
                tune.resident_lanes = (size_t)std::min(nb, 2) * 256 * (size_t)gpu->prop.multiProcessorCount;
            else (void)hipGetLastError();
            if (cur >= 0 && cur != gpu->hip_id) (void)hipSetDevice(cur);
        }
        if constexpr (G2_COOP_BUILT) { if (fp_d::NL >= 14) tune.long_runs = 1; }       // (the wave-pair accumulation's run lengths: msm_plan.hpp)
        if (stream == nullptr) {
            // a non-blocking private stream (a blocking one pays an implicit legacy-stream check on
            // every launch: +36 ms on a 2^26 MSM); join_default_stream() orders each call after the
            // work already queued on the legacy default stream instead
            HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&join_ev, hipEventDisableTiming));
            own_stream = true;
        }
    }
    ~msm_t()
    {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (cur != gpu->hip_id) (void)hipSetDevice(gpu->hip_id);
        (void)hipStreamSynchronize(stream);
        if (aux) (void)hipStreamSynchronize(aux);
        if (cpy) (void)hipStreamSynchronize(cpy);
        if (blob) (void)hipFree(blob);
        if (stage) (void)hipFree(stage);
        if (h_sums) (void)hipHostFree(h_sums);
        if (h_flag) (void)hipHostFree(h_flag);
        if (d_pflag) (void)hipFree(d_pflag);
        if (pre_points) (void)hipFree(pre_points);
        for (auto& e : tev) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_fork, ev_sorted[0], ev_sorted[1], ev_accdone[0], ev_accdone[1],
                             ev_copied[0], ev_copied[1], ev_chunkdone[0], ev_chunkdone[1], join_ev})
            if (e) (void)hipEventDestroy(e);
        if (aux) (void)hipStreamDestroy(aux);
        if (cpy) (void)hipStreamDestroy(cpy);
        if (own_stream) (void)hipStreamDestroy(stream);
        if (cur >= 0 && cur != gpu->hip_id) (void)hipSetDevice(cur);
    }
    msm_t(const msm_t&) = delete;
    msm_t& operator=(const msm_t&) = delete;

    int device() const { return gpu->hip_id; }
    void set_stream(hipStream_t s)
    {
        (void)hipStreamSynchronize(stream);
        if (own_stream) { (void)hipStreamDestroy(stream); own_stream = false; }
        stream = s;
        if (stream == nullptr) {
            HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            if (!join_ev) HIP_OK(hipEventCreateWithFlags(&join_ev, hipEventDisableTiming));
            own_stream = true;
        }
    }
    void enable_timing(bool on) { timing = on; }
    float kernel_ms(int which) const { return which >= 0 && which < 4 ? last_ms[which] : -1.f; }
    unsigned chunks_of_last_invoke() const { return last_chunks; }
    unsigned tail_redone() const { return last_redo; }
    size_t scratch_bytes() const { return blob_sz + stage_sz; }
    void release_scratch()
    {
        (void)hipSetDevice(gpu->hip_id);
        (void)hipStreamSynchronize(stream);
        if (aux) (void)hipStreamSynchronize(aux);
        if (cpy) (void)hipStreamSynchronize(cpy);
        if (blob) { (void)hipFree(blob); blob = nullptr; blob_sz = 0; }
        if (stage) { (void)hipFree(stage); stage = nullptr; stage_sz = 0; }
    }
    // ---- the scalars of one call: full width (FRp::NBITS bits in SCALAR_BYTES, folded below r/2 by k_breakdown), or SHORT:
    // |bits| declared significant bits, |stride| bytes apart (include/sppark_amd_short.h; k_breakdown_short) ----
    struct scalar_form {
        unsigned bits;                                  // 0 = full width
        size_t stride;
        scalar_form() : bits(0), stride(SCALAR_BYTES) {}
        scalar_form(unsigned b, size_t s) : bits(b), stride(s) {}
        unsigned plan_bits() const { return bits ? bits + 1 : (unsigned)FRp::NBITS; }    // (+ 1: the bit that closes the signed recoding)
    };
    static constexpr unsigned SHORT_BITS_MAX = FRp::NBITS - 2;
    // the contract of a short call; nothing but the arguments is looked at (no device, no memory)
    static void check_short(unsigned bits, size_t stride, const void* scalars)
    {
        const bool ok = bits >= 1 && bits <= SHORT_BITS_MAX && (stride & 3) == 0 && stride >= 4 * (size_t)((bits + 31) / 32) && stride <= 32
                        && ((size_t)scalars & (stride == 4 || stride == 8 || stride == 16 ? stride - 1 : 3)) == 0;
        if (!ok)
            throw hip_error(-(int)hipErrorInvalidValue, "short scalars: scalar_bits must be 1.." + std::to_string(SHORT_BITS_MAX)
                            + ", scalar_stride a multiple of 4 in [4 * ceil(scalar_bits / 32), 32], the scalars aligned to a stride of 4, 8 or 16 "
                              "bytes and to 4 bytes otherwise: invalid argument");
    }

    msm_plan plan_for(size_t npoints, unsigned short_bits = 0) const
    {   return make_plan(npoints, scalar_form(short_bits, 0).plan_bits(), tune);   }

    // Size the scratch for |npoints| ahead of time (so a timed invoke does not allocate).
    void reserve_for(size_t npoints, size_t ffi_affine_sz, bool host_points, bool host_scalars, const scalar_form& sf = scalar_form())
    {
        HIP_OK(hipSetDevice(gpu->hip_id));
        size_t chunk = choose_chunk(npoints, (host_points ? ffi_affine_sz : 0) + (host_scalars ? sf.stride : 0), sf.plan_bits());
        // as invoke(): one plan per chunk length, scratch for the largest layout
        const std::vector<size_t> cb = chunk_bounds(npoints, chunk);
        size_t need = 0;
        for (size_t c = 0; c + 1 < cb.size(); c++) need = std::max(need, make_layout(make_plan(cb[c + 1] - cb[c], sf.plan_bits(), tune), true).total);
        reserve(need);
        if (host_points || host_scalars)
            reserve_stage(2 * (align_up(host_points ? chunk * ffi_affine_sz : 0) + align_up(host_scalars ? chunk * sf.stride : 0)));
    }

    // Private stream only: wait for everything queued so far on the legacy default stream, where
    // most callers (PyTorch included) produce device-resident inputs.  Callers that work on other
    // streams pass theirs to the constructor / set_stream().
    void join_default_stream()
    {
        if (!own_stream) return;
        HIP_OK(hipEventRecord(join_ev, nullptr));
        HIP_OK(hipStreamWaitEvent(stream, join_ev, 0));
    }

    // Keep a copy of |np| points in HBM for later invoke(out, nullptr, n <= np, scalars, ...)
    // calls: the reference's msm_t(points, np, ffi_affine_sz) + invoke(out, scalars)
    // (pippenger.cuh:351-385,604-605).  |points| may be a host or a device pointer; np == 0 drops the copy.
    // window of the fixed-base tables: the c <= 26 with the least arithmetic -- W(c) * np mixed additions into the buckets
    // + two full additions (~3 mixed ones) for each of the 2^(c-1) buckets of the ONE bucket set (2^26 points: c = 24,
    // W = 11; c = 26, W = 10 costs the same and 4 x the buckets) -- or the forced width
    unsigned fixed_base_width(size_t np) const
    {
        if (tune.wbits) return std::min(26u, std::max(8u, tune.wbits));
        unsigned w = 0; double best = 0;
        for (unsigned c = 8; c <= 26; c++) {
            const double cost = (double)((FRp::NBITS - 1) / c + 1) * (double)np + 3.0 * (double)((size_t)1 << (c - 1));
            if (w == 0 || cost < best) { best = cost; w = c; }
        }
        return w;
    }
    // |fixed_base| (fields with their own records only): also keep the multiples 2^(off_j) * P_i of every point for
    // every window j (k_fixed_base_table), nwins x the memory; invoke(out, nullptr, np, ...) over exactly these np points
    // then runs as ONE window over nwins * np (digit, multiple) pairs -- fixed_plan() / invoke_fixed().
    void preload(const void* points, size_t np, size_t ffi_affine_sz, bool fixed_base = false)
    {
        HIP_OK(hipSetDevice(gpu->hip_id));
        HIP_OK(hipStreamSynchronize(stream));
        join_default_stream();
        // (arguments are checked before the previous set is dropped: a refused call leaves the context as it was)
        if (np != 0 && (points == nullptr || ffi_affine_sz < 2 * FP_BYTES || np > (1u << 31))) HIP_OK(hipErrorInvalidValue);
        if (np != 0 && fixed_base && !MONTX) HIP_OK(hipErrorNotSupported);
        if (np != 0 && fixed_base && (tune.wbits || np >= FIXED_BASE_MIN)
            && (size_t)((FRp::NBITS - 1) / fixed_base_width(np) + 1) * np >= ((size_t)1 << 31)) HIP_OK(hipErrorInvalidValue);
        if (pre_points) { HIP_OK(hipFree(pre_points)); pre_points = nullptr; pre_n = pre_stride = 0; }
        pre_fb_wbits = pre_fb_nwins = 0;
        if (np == 0) return;
        if (fixed_base && !MONTX) HIP_OK(hipErrorNotSupported);
        // measured (profiles/r03_msm_fixed_base.log): the one-window MSM wins from 2^24 points on and loses below 2^23
        // (the tables are gathered from HBM without reuse; the plain path's points are shared by all its windows).  Below the
        // threshold the call is a plain preload unless a window width was forced (tests, measurements).
        if (fixed_base && !tune.wbits && np < FIXED_BASE_MIN) fixed_base = false;
        unsigned fb_w = 0, fb_nw = 1;
        if (fixed_base) {
            fb_w = fixed_base_width(np);
            fb_nw = (FRp::NBITS - 1) / fb_w + 1;
            fb_w = FRp::NBITS / fb_nw + (FRp::NBITS % fb_nw ? 1 : 0);
            if ((size_t)fb_nw * np >= ((size_t)1 << 31)) HIP_OK(hipErrorInvalidValue);
        }
        if (points == nullptr || ffi_affine_sz < 2 * FP_BYTES || np > (1u << 31)) HIP_OK(hipErrorInvalidValue);
        struct dev_buf {                // staging copy of host-resident points: freed on every exit path
            unsigned char* p = nullptr;
            ~dev_buf() { if (p) (void)hipFree(p); }
        } staging;
        try {
            if constexpr (INTERNAL) {
                // bases are constant across invocations: convert them into the field's own records once
                const unsigned char* src = (const unsigned char*)points;
                if (!is_device_pointer(points)) {
                    HIP_OK(hipMalloc((void**)&staging.p, np * ffi_affine_sz));
                    HIP_OK(hipMemcpyAsync(staging.p, points, np * ffi_affine_sz, hipMemcpyHostToDevice, stream));
                    src = staging.p;
                }
                HIP_OK(dev_scratch_pool::malloc_or_drain((void**)&pre_points, (size_t)fb_nw * np * conv_stride()));
                launch_convert(pre_points, src, (unsigned)np, ffi_affine_sz);
                if constexpr (MONTX) if (fixed_base) {
                    hipLaunchKernelGGL(k_fixed_base_table<fp_d>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream,
                                       pre_points, (unsigned)np, fb_nw, (unsigned)FRp::NBITS);
                    HIP_OK(hipGetLastError());
                }
            } else {
                HIP_OK(hipMalloc((void**)&pre_points, np * ffi_affine_sz));
                HIP_OK(hipMemcpyAsync(pre_points, points, np * ffi_affine_sz,
                                      is_device_pointer(points) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
            }
            HIP_OK(hipStreamSynchronize(stream));
        } catch (...) {
            if (pre_points) { (void)hipFree(pre_points); pre_points = nullptr; }
            throw;
        }
        pre_n = np; pre_stride = ffi_affine_sz;
        if (fixed_base) { pre_fb_wbits = fb_w; pre_fb_nwins = fb_nw; }
    }
    unsigned fixed_base_windows() const { return pre_fb_nwins; }
    size_t preloaded() const { return pre_n; }

private:
    static void no_kernel() { HIP_OK(hipErrorInvalidDeviceFunction); }      // the route named a kernel this field does not have
    // wire points -> the field's own records, by the kernel the route chooses (route_convert)
    void launch_convert(unsigned char* dst, const unsigned char* src, unsigned n, size_t stride, hipStream_t on = nullptr)
    {
        if constexpr (INTERNAL)
            issue_convert(route_convert(field(), tune.sw, n, stride, ((size_t)src & 15) == 0), dst, src, stride, on ? on : stream);
    }
    void issue_convert(const msm_step& s, unsigned char* dst, const unsigned char* src, size_t stride, hipStream_t on)
    {
        if constexpr (INTERNAL) {
            const dim3 grid(s.gx), block(s.block);
            switch (s.kernel) {
            case MK_CONVERT:         hipLaunchKernelGGL((k_convert_points<fp_d, false>), grid, block, 0, on, dst, src, s.count, (unsigned)stride); break;
            case MK_CONVERT_FLAGGED: hipLaunchKernelGGL((k_convert_points<fp_d, true>), grid, block, 0, on, dst, src, s.count, (unsigned)stride); break;
            case MK_CONVERT_STAGED:
                if constexpr (MONTX) hipLaunchKernelGGL((k_convert_points_staged<fp_d, false>), grid, block, 0, on, dst, src, s.count); else no_kernel();
                break;
            case MK_CONVERT_STAGED_FLAGGED:
                if constexpr (MONTX) hipLaunchKernelGGL((k_convert_points_staged<fp_d, true>), grid, block, 0, on, dst, src, s.count); else no_kernel();
                break;
            default: no_kernel();
            }
            HIP_OK(hipGetLastError());
        } else no_kernel();
    }

    // points per chunk.  |stage_per_point|: bytes of host-resident input per point that have to be
    // copied (0: everything is on the device); chunking then overlaps the copies with the
    // arithmetic.  Device-resident inputs are chunked only when the scratch would not fit.
    // |plan_bits|: the scalar bits the chunks are planned for (scalar_form::plan_bits)
    size_t choose_chunk(size_t n, size_t stage_per_point, unsigned plan_bits = FRp::NBITS) const
    {
        size_t chunk = n;
        if (tune.chunk) chunk = std::min(n, std::max<size_t>(tune.chunk, 1));
        else if (stage_per_point && n > ((size_t)1 << 21)) {
            // 4 chunks of 2^20..2^24 points: the exposed first copy and last computation are 1/4 of
            // the total each, and every chunk is still an efficient MSM (a chunk pays its own bucket
            // sums: 2^21-point chunks cost 2^24 points 87 ms, 2^22-point chunks 75 ms;
            // profiles/r02_msm_host_path.log)
            chunk = std::min<size_t>(std::max<size_t>(n / 4, (size_t)1 << 20), (size_t)1 << 24);
        }
        auto need = [&](size_t c) {
            return make_layout(make_plan(c, plan_bits, tune), true).total + 2 * c * stage_per_point + 1024;
        };
        size_t limit = tune.max_scratch;
        if (!limit) {
            // already reserved (both allocations, each on its own: the scratch blob and the staging sets
            // are separate hipMallocs): no driver query
            const bool blob_ok = make_layout(make_plan(chunk, plan_bits, tune), true).total <= blob_sz;
            const bool stage_ok = stage_per_point == 0 || 2 * (chunk * stage_per_point + 512) <= stage_sz;  // two sets, each of two 256-byte aligned parts
            if (blob_ok && stage_ok) return chunk;
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return chunk; }
            limit = free_b - (free_b >> 5) + blob_sz + stage_sz;        // what this context may hold in total
        }
        while (need(chunk) > limit && chunk > 4096) chunk = (chunk + 1) / 2;
        return chunk;
    }

    // Chunk boundaries [b_0 = 0, b_1, ..., b_k = n]: equal chunks, the last one shorter.
    // (Round 4 measured the alternatives for host-resident inputs on a host whose pinned H2D rate is 57 GB/s,
    // profiles/r04_msm_host_path.log: the pipeline behaves exactly like t = sum over chunks of max(copy, compute of the
    // previous chunk) + the last computation, with the copies AT the link rate -- 2^26 points: 163 ms of copies + one
    // exposed 2^24-point MSM = 201 ms.  Half-sized first / last chunks change nothing (the second-to-last computation is
    // exposed instead: 202 ms); the points copy in 2 or 4 slices from as many host threads and streams changes nothing
    // (201 ms: one pageable copy already saturates the link); eight 2^23-point chunks gain 5 % here (190 ms) and lost
    // 8 % on the host of round 3 (266 vs 245 ms, profiles/r03_msm_host_path.log), where small pageable copies are
    // slower per byte.  So: four chunks of at most 2^24 points, as the reference's 2^24-point strides.)
    std::vector<size_t> chunk_bounds(size_t n, size_t chunk) const
    {
        std::vector<size_t> b{0};
        for (size_t lo = chunk; lo < n; lo += chunk) b.push_back(lo);
        b.push_back(n);
        return b;
    }

    // ---- one complete MSM over device-resident data, asynchronously on stream (+ aux) ----------
    // d_points: wire points (stride, flagged) or, when preconverted, the field's own records.
    // h_out: nwins window sums in pinned host memory, valid once |stream| has been synchronised.
    // |fb_n| != 0: fixed-base mode -- |p| describes ONE window over fb_nwins * fb_n entries; the digits come from the
    // fb_n scalars cut into fb_nwins real windows (digit (w, i) is entry w * fb_n + i of the one window)
    void sort_group(hipStream_t ss, const msm_plan& p, const layout& l, unsigned b, unsigned w0, unsigned wn,
                    const u32* d_scalars, bool mont, unsigned fb_n = 0, unsigned fb_nwins = 0, const scalar_form& form = scalar_form())
    {
        u32* digits = (u32*)(blob + l.digits[b]);
        u32* sorted = (u32*)(blob + l.sorted[b]);
        u32* H = (u32*)(blob + l.H[b]);
        u32* tot = (u32*)(blob + l.tot[b]);
        u32* off = (u32*)(blob + l.off[b]);
        void* partA = blob + l.partA[b];
        u32* offA = (u32*)(blob + l.offA[b]);
        // level-A records: 4 bytes where the plan allows it (msm_sort_kernels.hpp), PK = packed
        const bool packed = p.IB != 0;
        unsigned ngp = 1; while (ngp < p.NG) ngp <<= 1;
        const partA_fmt fmt{H, p.IB, p.SH, ngp, p.nslabs};
        // local index of the first short window of this group (window_len: the first nbits % nwins are long)
        const unsigned nlong = p.nbits % p.nwins, sf = nlong == 0 ? wn : (nlong > w0 ? std::min(wn, nlong - w0) : 0u);
        if (fb_n) {
            unsigned grid = std::min<unsigned>((fb_n + 255) / 256, 256 * 16);
            hipLaunchKernelGGL(k_breakdown<fr_d>, dim3(grid), dim3(256), 0, ss,
                               digits, d_scalars, fb_n, fb_nwins, (unsigned)FRp::NBITS, (int)mont, 0u, fb_nwins);
        } else if (form.bits) {
            // short scalars: the plan's nbits is form.bits + 1; instantiated by the words that hold the bits, rounded up to 1, 2, 4, 8
            const unsigned grid = std::min<unsigned>((p.n + 255) / 256, 256 * 16), sw = (unsigned)(form.stride / 4);
            const dim3 g(grid), t(256);
            switch (short_words_pow2((form.bits + 31) / 32)) {
            case 1:  hipLaunchKernelGGL(k_breakdown_short<1>, g, t, 0, ss, digits, d_scalars, p.n, p.nwins, p.nbits, sw, w0, wn); break;
            case 2:  hipLaunchKernelGGL(k_breakdown_short<2>, g, t, 0, ss, digits, d_scalars, p.n, p.nwins, p.nbits, sw, w0, wn); break;
            case 4:  hipLaunchKernelGGL(k_breakdown_short<4>, g, t, 0, ss, digits, d_scalars, p.n, p.nwins, p.nbits, sw, w0, wn); break;
            default: hipLaunchKernelGGL(k_breakdown_short<8>, g, t, 0, ss, digits, d_scalars, p.n, p.nwins, p.nbits, sw, w0, wn); break;
            }
        } else {
            unsigned grid = std::min<unsigned>((p.n + 255) / 256, 256 * 16);
            hipLaunchKernelGGL(k_breakdown<fr_d>, dim3(grid), dim3(256), 0, ss,
                               digits, d_scalars, p.n, p.nwins, p.nbits, (int)mont, w0, wn);
        }
        HIP_OK(hipGetLastError());
        size_t ldsA = (size_t)p.NA * 4, ldsB = ((size_t)1 << p.LB) * 4 + SORT_NT * 4 + (size_t)SORTB_STAGE * 4 + PARTA_MAX_GROUPS * 4;
        // (the attribute is per device and sticky: raised once to the largest size asked for so far,
        // not on every MSM -- lds_attr())
        if (ldsA > 65536) { lds_attr((const void*)k_histA, ldsA); lds_attr(packed ? (const void*)k_scatterA<true> : (const void*)k_scatterA<false>, ldsA); }
        if (ldsB > 65536) lds_attr(packed ? (const void*)k_sortB<true> : (const void*)k_sortB<false>, ldsB);
        hipLaunchKernelGGL(k_histA, dim3(p.nslabs, wn), dim3(SORT_NT), ldsA, ss,
                           H, digits, p.n, p.nslabs, p.slab_sz, p.NA, p.LB, sf);
        HIP_OK(hipGetLastError());
        size_t na_total = (size_t)wn * p.NA;
        hipLaunchKernelGGL(k_scan_slabs, dim3((unsigned)((na_total + 255) / 256)), dim3(256), 0, ss,
                           H, tot, p.nslabs, p.NA, wn);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(k_scan_parts, dim3(wn), dim3(1024), 0, ss, offA, tot, p.NA);
        HIP_OK(hipGetLastError());
        if (p.NA <= SCATA_MAX_NA && p.LB < 16) {      // (always, with the automatic split: HB <= 12)
            const size_t ldsS = scatterA_staged_lds(p.NA);
            lds_attr(packed ? (const void*)k_scatterA_staged<true> : (const void*)k_scatterA_staged<false>, ldsS);
            if (packed) hipLaunchKernelGGL(k_scatterA_staged<true>, dim3(p.nslabs, wn), dim3(SORT_NT), ldsS, ss,
                                           (u32*)partA, digits, H, offA, p.n, p.nslabs, p.slab_sz, p.NA, p.LB, sf, p.IB);
            else        hipLaunchKernelGGL(k_scatterA_staged<false>, dim3(p.nslabs, wn), dim3(SORT_NT), ldsS, ss,
                                           (uint2*)partA, digits, H, offA, p.n, p.nslabs, p.slab_sz, p.NA, p.LB, sf, p.IB);
        } else {
            if (packed) hipLaunchKernelGGL(k_scatterA<true>, dim3(p.nslabs, wn), dim3(SORT_NT), ldsA, ss,
                                           (u32*)partA, digits, H, offA, p.n, p.nslabs, p.slab_sz, p.NA, p.LB, sf, p.IB);
            else        hipLaunchKernelGGL(k_scatterA<false>, dim3(p.nslabs, wn), dim3(SORT_NT), ldsA, ss,
                                           (uint2*)partA, digits, H, offA, p.n, p.nslabs, p.slab_sz, p.NA, p.LB, sf, p.IB);
        }
        HIP_OK(hipGetLastError());
        const unsigned big = tune.big ? tune.big : p.big ? p.big : (1u << 18);
        u32* nbig = (u32*)(blob + l.bigl[b]); u32* blist = nbig + 1; u32* curB = (u32*)(blob + l.curB[b]);
        // (a window of n entries cannot hold a partition above |big| when n <= big: the list of oversized partitions and its
        // three kernels -- which would find nothing and return, ~5 us of launch each -- are not even queued: 25 us of every
        // MSM up to 2^18 points)
        const bool may_be_big = p.n > big;
        if (may_be_big) HIP_OK(hipMemsetAsync(nbig, 0, 4, ss));
        if (packed) hipLaunchKernelGGL(k_sortB<true>, dim3(p.NA, wn), dim3(SORT_NT), ldsB, ss,
                                       sorted, off, (const u32*)partA, offA, p.n, p.NA, p.LB, sf, big, fmt);
        else        hipLaunchKernelGGL(k_sortB<false>, dim3(p.NA, wn), dim3(SORT_NT), ldsB, ss,
                                       sorted, off, (const uint2*)partA, offA, p.n, p.NA, p.LB, sf, big, fmt);
        HIP_OK(hipGetLastError());
        if (!may_be_big) return;
        // oversized partitions (skewed scalars); empty list and immediate return otherwise
        hipLaunchKernelGGL(k_big_find, dim3((p.NA * wn + 255) / 256), dim3(256), 0, ss,
                           nbig, blist, off, offA, p.NA, p.LB, sf, wn, big);
        size_t ldsBig = ((size_t)1 << p.LB) * 4;
        // slices per listed partition: 64 (one whole window in a partition), or about half of what k_big_scatter stages
        // in LDS when the AVERAGE partition is already near the threshold (the one-window plan of the fixed-base mode,
        // whose partitions differ by a factor of two)
        const size_t avg = (size_t)p.n / p.NA;
        const unsigned split = avg > big / 2 ? (unsigned)std::min<size_t>(SORTB_SPLIT, avg / (BIG_STAGE / 2) + 1) : SORTB_SPLIT;
        if (packed) hipLaunchKernelGGL(k_big_hist<true>, dim3(1024), dim3(1024), ldsBig, ss, off, (const u32*)partA, offA, nbig, blist, p.n, p.NA, p.LB, sf, split);
        else        hipLaunchKernelGGL(k_big_hist<false>, dim3(1024), dim3(1024), ldsBig, ss, off, (const uint2*)partA, offA, nbig, blist, p.n, p.NA, p.LB, sf, split);
        hipLaunchKernelGGL(k_big_scan, dim3(p.NA > 64 && avg > big / 2 ? 1024 : 64), dim3(1024), 0, ss, off, curB, offA, nbig, blist, p.NA, p.LB, sf);
        const size_t ldsSc = big_scatter_lds(p.LB);
        if (ldsSc > 65536) lds_attr(packed ? (const void*)k_big_scatter<true> : (const void*)k_big_scatter<false>, ldsSc);
        if (packed) hipLaunchKernelGGL(k_big_scatter<true>, dim3(1024), dim3(1024), ldsSc, ss, sorted, curB, (const u32*)partA, offA, nbig, blist, p.n, p.NA, p.LB, sf, split, fmt);
        else        hipLaunchKernelGGL(k_big_scatter<false>, dim3(1024), dim3(1024), ldsSc, ss, sorted, curB, (const uint2*)partA, offA, nbig, blist, p.n, p.NA, p.LB, sf, split, fmt);
        HIP_OK(hipGetLastError());
    }

    // The kernels between the sort and the copy of the window sums are what the ROUTE says (msm_route.hpp make_route): this
    // function keeps the streams and events, the per-group sort and accumulation loop, the memsets and the copies.
    // |redo|: only the fan-in tree over the records the piece tree left, and everything after it (invoke(), when the flag of
    // the first pass says that a bucket had more pieces than the piece tree was sized for)
    // (|may_defer|: the caller looks at the flag after this MSM -- invoke() with one chunk)
    void enqueue(const msm_plan& p, const layout& l, const unsigned char* d_points, size_t stride, bool preconverted,
                 const u32* d_scalars, bool mont, std_bucket_t* h_out, bool first_timed, unsigned fb_n = 0, unsigned fb_nwins = 0,
                 bool redo = false, bool may_defer = false, const scalar_form& sf = scalar_form())
    {
        msm_call call;
        call.fb_n = fb_n; call.redo = redo; call.may_defer = may_defer; call.short_bits = sf.bits;
        call.convert = INTERNAL && !preconverted;
        call.flagged = !preconverted && stride > 2 * FP_BYTES;
        call.stride = stride; call.aligned16 = ((size_t)d_points & 15) == 0;
#ifdef SPPARK_TUNING
        if (const char* e = getenv("SPPARK_TOP_CUT")) call.top_cut = (unsigned)atoi(e);        // "sb sp" as two digits, e.g. 24 (sweeps only)
#endif
        const msm_route route = make_route(p, tune, field(), call);
        if (route.overflow) HIP_OK(hipErrorInvalidValue);
        const bool multi = p.G > 1;
        if (multi) need_aux();
        if (timing && first_timed && !redo) { need_tev(2 + 2 * p.G); HIP_OK(hipEventRecord(tev[0], stream)); }
        if (multi) {                                // the inputs are ready at this point of the main stream
            HIP_OK(hipEventRecord(ev_fork, stream));
            HIP_OK(hipStreamWaitEvent(aux, ev_fork, 0));
        }
        bucket_t* buckets = (bucket_t*)(blob + l.buckets);
        std_bucket_t* fin = (std_bucket_t*)(blob + l.sums);
        const u32* off0 = (const u32*)(blob + l.off[0]);
        // the route's buffer roles as pointers
        auto rec = [&](msm_buf b) -> bucket_t* {
            switch (b) {
            case MB_BUCKETS: return buckets;
            case MB_PT_A: return (bucket_t*)(blob + l.ptA);
            case MB_PT_B: return (bucket_t*)(blob + l.ptB);
            case MB_A1: return (bucket_t*)(blob + l.A1);
            case MB_W1: return (bucket_t*)(blob + l.W1);
            case MB_A2: return (bucket_t*)(blob + l.A2);
            case MB_W2: return (bucket_t*)(blob + l.W2);
            default: return nullptr;
            }
        };
        auto key = [&](msm_buf b) -> u32* {
            return (u32*)(b == MB_KEY_A ? blob + l.keyA : b == MB_KEY_B ? blob + l.keyB : b == MB_KEY_C ? blob + l.keyC : nullptr);
        };
        auto flag_word = [&](msm_flag f) -> u32* { return f == MF_SCRATCH ? (u32*)(blob + l.flag) : f == MF_SMALL ? d_pflag : nullptr; };
        // one step of the route: roles -> pointers, and the launch.  (|w0|, |wn|, |b|: the window group and sort set of an accumulation)
        auto launch = [&](const msm_step& s, unsigned w0 = 0, unsigned wn = 0, unsigned b = 0) {
            const dim3 grid(s.gx, s.gy), block(s.block);
            bucket_t *r0 = rec(s.rd[0]), *r1 = rec(s.rd[1]), *w0p = rec(s.wr[0]), *w1p = rec(s.wr[1]);
            u32* flag = flag_word(s.flag);
            const u32* offp = multi ? (const u32*)nullptr : off0;       // (one group: empty buckets are recognised from the offsets)
#define SPPARK_GO(kernel, ...) hipLaunchKernelGGL((kernel), grid, block, s.lds, stream, __VA_ARGS__)
#define SPPARK_GO_G1(kernel, ...) do { if constexpr (MONTX) SPPARK_GO(kernel, __VA_ARGS__); else no_kernel(); } while (0)
            switch (s.kernel) {
            case MK_CONVERT: case MK_CONVERT_FLAGGED: case MK_CONVERT_STAGED: case MK_CONVERT_STAGED_FLAGGED:
                issue_convert(s, blob + l.conv, d_points, stride, stream);
                return;
            // (fields with their own records read them at their own stride and ignore this one)
            case MK_ACCUMULATE: case MK_ACCUMULATE_FLAGGED: case MK_ACCUMULATE_G2C: {
                const u32* sorted = (const u32*)(blob + l.sorted[b]);
                const u32* off = (const u32*)(blob + l.off[b]);
                const dim3 rows(s.gx, wn);
                u32* keyA = key(MB_KEY_A); bucket_t* ptA = rec(MB_PT_A);
                if (s.kernel == MK_ACCUMULATE_G2C) {
                    if constexpr (G2_COOP_BUILT)
                        hipLaunchKernelGGL((k_accumulate_g2c<fp_d>), rows, block, 0, stream, buckets, keyA, ptA, d_points, (unsigned)stride,
                                           sorted, off, p.n, p.NB, p.L, p.chunks_per_win, w0);
                    else no_kernel();
                } else if (s.kernel == MK_ACCUMULATE_FLAGGED)
                    hipLaunchKernelGGL((k_accumulate<fp_d, true>), rows, block, 0, stream, buckets, keyA, ptA, d_points, (unsigned)stride,
                                       sorted, off, p.n, p.NB, p.L, p.chunks_per_win, w0);
                else
                    hipLaunchKernelGGL((k_accumulate<fp_d, false>), rows, block, 0, stream, buckets, keyA, ptA, d_points, (unsigned)stride,
                                       sorted, off, p.n, p.NB, p.L, p.chunks_per_win, w0);
                break;
            }
            case MK_PIECE_LEVEL:
                SPPARK_GO(k_piece_level<fp_d>, buckets, key(s.rd[0]), r1, off0, p.NB, p.L, p.chunks_per_win, p.nwins, route.piece_cmax, s.t, s.last, flag);
                break;
            case MK_PIECE_LEVEL_COOP:
                SPPARK_GO_G1(k_piece_level_coop<fp_d>, buckets, key(s.rd[0]), r1, off0, p.NB, p.L, p.chunks_per_win, p.nwins, route.piece_cmax, s.t, s.last, flag);
                break;
            case MK_PIECE_TAIL_COOP:
                SPPARK_GO_G1(k_piece_tail_coop<fp_d>, buckets, key(s.rd[0]), r1, off0, p.NB, p.L, p.chunks_per_win, p.nwins, route.piece_cmax, s.t, s.lgGB, flag);
                break;
            case MK_JOIN_RUNS:
                HIP_OK(hipMemsetAsync(flag, 0, 4, stream));
                SPPARK_GO(k_join_runs<fp_d>, buckets, key(s.wr[0]), key(s.rd[0]), r1, s.count, flag);
                break;
            case MK_REDUCE_RUNS:
                SPPARK_GO(k_reduce_runs<fp_d>, buckets, key(s.wr[0]), w1p, key(s.rd[0]), r1, s.count, s.fan, s.nthreads, (int)s.last, (const u32*)flag);
                break;
            case MK_REDUCE_RUNS_COOP:
                SPPARK_GO_G1(k_reduce_runs_coop<fp_d>, buckets, key(s.wr[0]), w1p, key(s.rd[0]), r1, s.count, s.fan, s.nthreads, 0, (const u32*)flag);
                break;
            case MK_REDUCE_TAIL:
                SPPARK_GO(k_reduce_tail<fp_d>, buckets, key(s.rd[0]), r1, key(s.wr[0]), w1p, s.count, s.fan, (const u32*)flag);
                break;
            case MK_REDUCE_TAIL_COOP:
                SPPARK_GO_G1(k_reduce_tail_coop<fp_d>, buckets, key(s.rd[0]), r1, key(s.wr[0]), w1p, s.count, s.fan, (const u32*)flag);
                break;
            case MK_BUCKET_SMALL_BITS_COOP: SPPARK_GO_G1(k_bucket_small_bits_coop<fp_d>, w0p, buckets, off0, p.NB, s.m); break;
            case MK_BUCKET_LEVEL1:      SPPARK_GO(k_bucket_level1<fp_d>, w0p, w1p, buckets, p.NB, s.fan, p.nwins, offp); break;
            case MK_BUCKET_LEVEL1_LAT:  SPPARK_GO_G1(k_bucket_level1_lat<fp_d>, w0p, w1p, buckets, p.NB, s.fan, p.nwins, offp); break;
            case MK_BUCKET_LEVEL1_PIPE: SPPARK_GO_G1(k_bucket_level1_pipe<fp_d>, w0p, w1p, buckets, p.NB, s.fan, p.nwins, offp); break;
            case MK_BUCKET_LEVEL1_COOP: SPPARK_GO_G1(k_bucket_level1_coop<fp_d>, w0p, w1p, buckets, p.NB, s.fan, p.nwins, offp); break;
            case MK_BUCKET_LEVELN:      SPPARK_GO(k_bucket_levelN<fp_d>, w0p, w1p, r0, r1, s.count, s.fan, s.lgG, p.nwins); break;
            case MK_BUCKET_LEVELN_LAT:  SPPARK_GO_G1(k_bucket_levelN_lat<fp_d>, w0p, w1p, r0, r1, s.count, s.fan, s.lgG, p.nwins); break;
            case MK_BUCKET_LEVELN_PIPE: SPPARK_GO_G1(k_bucket_levelN_pipe<fp_d>, w0p, w1p, r0, r1, s.count, s.fan, s.lgG, p.nwins); break;
            case MK_BUCKET_LEVELN_COOP: SPPARK_GO_G1(k_bucket_levelN_coop<fp_d>, w0p, w1p, r0, r1, s.count, s.fan, s.lgG, p.nwins); break;
            case MK_BUCKET_TOP_BITS:
                if (s.lds > 65536) lds_attr((const void*)k_bucket_top_bits<fp_d>, s.lds);
                SPPARK_GO(k_bucket_top_bits<fp_d>, w0p, r0, r1, s.count, s.m, s.lgG);
                break;
            case MK_BUCKET_TOP_SUM: SPPARK_GO(k_bucket_top_sum<fp_d>, w0p, r0, s.m); break;
            case MK_BUCKET_TOP_BITS_COOP:
                if constexpr (MONTX) { if (s.lds > 65536) lds_attr((const void*)k_bucket_top_bits_coop<fp_d>, s.lds); }
                SPPARK_GO_G1(k_bucket_top_bits_coop<fp_d>, w0p, r0, r1, s.count, s.m, s.lgG, s.sb, s.sp);
                break;
            case MK_BUCKET_TOP_SUM_COOP:        // (the wire image with it, and the small sizes' flag behind the sums)
                SPPARK_GO_G1(k_bucket_top_sum_coop<fp_d>, w0p, r0, s.count, fin, flag, flag ? reinterpret_cast<u32*>(fin + p.nwins) : (u32*)nullptr);
                break;
            case MK_FINALIZE:
                if constexpr (INTERNAL) SPPARK_GO((k_finalize<fp_d, STD_WORDS>), fin, r0, p.nwins); else no_kernel();
                break;
            default: no_kernel();
            }
#undef SPPARK_GO_G1
#undef SPPARK_GO
            HIP_OK(hipGetLastError());
        };
        // With ONE window group the bucket offsets of every window are still there when the bucket sums run:
        // empty buckets are recognised from them and never read (k_bucket_level1), so no memset.  With several
        // groups the two offset sets are reused, and the buckets are cleared instead.
        if (multi && !redo) HIP_OK(hipMemsetAsync(buckets, 0, (size_t)p.nwins * p.NB * sizeof(bucket_t), stream));

        for (unsigned g = 0; g < p.G && !redo; g++, gseq++) {
            // sort sets by the parity of a counter that keeps running across MSMs (chunks): the
            // events of set b then always refer to the previous user of set b
            const unsigned b = multi ? (gseq & 1) : 0, w0 = g * p.wpg, wn = std::min(p.wpg, p.nwins - w0);
            if (g == 0) {
                // first group: on the main stream, at full width (stream order protects the set)
                sort_group(stream, p, l, b, w0, wn, d_scalars, mont, fb_n, fb_nwins, sf);
                // (the conversion does not depend on the scalars, but running it on the second stream beside the digit /
                // sort kernels gains nothing: all of them are memory-bound and share HBM -- 13.4 ms before the accumulation
                // either way at 2^26, profiles/r04_msm_convert_beside_sort_negative.log; round 2 measured the same)
                if (call.convert) {                 // wire points -> the field's own records (2 products per point)
                    launch(route.steps[0]);
                    d_points = blob + l.conv;
                }
            } else {
                if (gseq >= 2) HIP_OK(hipStreamWaitEvent(aux, ev_accdone[b], 0));    // the accumulation two groups back has read this set
                sort_group(aux, p, l, b, w0, wn, d_scalars, mont, 0, 0, sf);
                HIP_OK(hipEventRecord(ev_sorted[b], aux));
                HIP_OK(hipStreamWaitEvent(stream, ev_sorted[b], 0));
            }
            if (timing && first_timed) HIP_OK(hipEventRecord(tev[2 + 2 * g], stream));
            launch(route.steps[route.front - 1], w0, wn, b);
            if (timing && first_timed) HIP_OK(hipEventRecord(tev[3 + 2 * g], stream));
            if (multi) HIP_OK(hipEventRecord(ev_accdone[b], stream));
        }

        // ---- the tail: [piece tree |] record tree, bucket sums -- msm_route.hpp says which, and why ----
        unsigned si = route.front;
        piece_pending = route.piece_pending;
        if (route.flag_with_sums && !d_pflag) {
            HIP_OK(hipMalloc((void**)&d_pflag, 64));
            HIP_OK(hipMemsetAsync(d_pflag, 0, 64, stream));
        }
        if (route.pieces) {
            // the flag word the piece steps raise: the scratch blob's is cleared here and copied back on its own; the small
            // sizes' is zero already and comes back behind the window sums
            const msm_flag which = route.steps[si].flag;
            u32* flag = flag_word(which);
            if (which == MF_SCRATCH) HIP_OK(hipMemsetAsync(flag, 0, 4, stream));
            for (const unsigned end = si + route.pieces; si < end; si++) launch(route.steps[si]);
            if (!h_flag) HIP_OK(hipHostMalloc((void**)&h_flag, 64, hipHostMallocDefault));
            if (which == MF_SCRATCH) HIP_OK(hipMemcpyAsync(h_flag, flag, 4, hipMemcpyDeviceToHost, stream));
            h_flag_cur = which == MF_SMALL ? reinterpret_cast<const u32*>(h_out + p.nwins) : h_flag;
        }
        for (; si < route.nsteps && route.steps[si].kernel != MK_FINALIZE; si++) launch(route.steps[si]);
        if (timing && first_timed && !redo) HIP_OK(hipEventRecord(tev[1], stream));
        // ---- device -> host: one XYZZ per window (wire image); Horner on the host ------------------
        if constexpr (INTERNAL) {
            if (si < route.nsteps) launch(route.steps[si]);         // k_finalize, where no step wrote the wire image
            HIP_OK(hipMemcpyAsync(h_out, fin, (p.nwins + (route.flag_with_sums ? 1 : 0)) * sizeof(std_bucket_t), hipMemcpyDeviceToHost, stream));
        } else {
            HIP_OK(hipMemcpyAsync(h_out, rec(route.result), p.nwins * sizeof(std_bucket_t), hipMemcpyDeviceToHost, stream));
        }
    }

public:
    // pieces per bucket the piece tree of a small MSM takes (msm_route.hpp piece_tree_cmax), 0 = none
    unsigned piece_tree_cmax(const msm_plan& p, unsigned short_bits = 0) const
    {   return sppark_amd::piece_tree_cmax(p, tune.sw, 0, FRp::MOD, (unsigned)FRp::N, short_bits);   }
private:

    // Horner over the window sums (the reference's host-side collect, pippenger.cuh:627-727, is O(256 * windows))
    static point_t horner(const std_bucket_t* sums, const msm_plan& p)
    {
        point_t out; out.set_inf();
        for (unsigned w = p.nwins; w--;) {
            fp_h c[4];
            memcpy(c, &sums[w], sizeof(c));
            point_t s = point_t::from_xyzz(c[0], c[1], c[2], c[3]);
            out.add(s);
            if (w) for (unsigned k = 0; k < window_len(w - 1, p.nwins, p.nbits); k++) out.dbl();
        }
        return out;
    }

    // The plan of a fixed-base MSM: ONE window of |wbits| bits over fb_nwins * n entries (the multiples are baked into
    // the table, so every window's digits select from one bucket set).
    msm_plan fixed_plan(size_t n) const
    {   return make_fixed_plan(n, pre_fb_wbits, pre_fb_nwins, SORTB_STAGE, tune);   }

    // The one-window layout of the fixed-base mode needs ~16 B x windows x n of sort scratch in ONE piece (it cannot be
    // chunked: the tables cover the whole vector).  When the device cannot hold it next to the tables, invoke() runs the
    // ordinary chunked path on level 0 of the table instead of failing.
    bool fixed_fits(size_t npoints, const void* scalars) const
    {
        const size_t need = make_layout(fixed_plan(npoints), false).total
                          + (is_device_pointer(scalars) ? 0 : 2 * align_up(npoints * SCALAR_BYTES));
        if (need <= blob_sz + stage_sz) return true;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return true; }
        return need <= free_b - (free_b >> 5) + blob_sz + stage_sz;
    }

    // out = sum s_i * P_i over the preloaded points through their fixed-base tables: device-resident scalars or host
    // scalars (copied in one piece), one pass, one window.
    void invoke_fixed(point_t& out, size_t npoints, const void* scalars, bool mont)
    {
        const msm_plan p = fixed_plan(npoints);
        const layout l = make_layout(p, false);
        const bool sc_dev = is_device_pointer(scalars);
        reserve(l.total);
        reserve_sums(MAX_WINS);
        const u32* d_scalars = (const u32*)scalars;
        if (!sc_dev) {
            reserve_stage(2 * align_up(npoints * SCALAR_BYTES));
            HIP_OK(hipMemcpyAsync(stage, scalars, npoints * SCALAR_BYTES, hipMemcpyHostToDevice, stream));
            d_scalars = (const u32*)stage;
        }
        enqueue(p, l, pre_points, conv_stride(), true, d_scalars, mont, h_sums, true, (unsigned)npoints, pre_fb_nwins);
        HIP_OK(hipStreamSynchronize(stream));
        last_chunks = 1;
        if (timing) {
            float acc = 0;
            HIP_OK(hipEventElapsedTime(&acc, tev[2], tev[3]));
            HIP_OK(hipEventElapsedTime(&last_ms[0], tev[0], tev[2]));
            last_ms[1] = acc;
            HIP_OK(hipEventElapsedTime(&last_ms[2], tev[0], tev[1]));
            last_ms[3] = 1.f;
        }
        out = horner(h_sums, p);                            // one window: its sum is the result
    }

public:
    // Bitmap batch addition (msm/batch_addition.cuh:25-132): out = sum of the selected points.
    // points / bitmap / refmap (nullable): host or device pointers; maps are ceil(n/32) words.
    void batch_add(point_t& out, const void* points, size_t npoints, const uint32_t* bitmap, const uint32_t* refmap,
                   size_t ffi_affine_sz)
    {
        out.set_inf();
        if (npoints == 0) return;
        if (npoints > (1u << 31) || !points || !bitmap || ffi_affine_sz < 2 * FP_BYTES) HIP_OK(hipErrorInvalidValue);
        HIP_OK(hipSetDevice(gpu->hip_id));
        join_default_stream();
        const size_t nwords = (npoints + 31) / 32;
        const unsigned span = 4;                                    // 128 points per lane
        const size_t nrec = (nwords + span - 1) / span, F = 8;
        size_t o = 0;
        auto take = [&](size_t sz) { size_t r = o; o += align_up(sz); return r; };
        const bool pts_dev = is_device_pointer(points), bm_dev = is_device_pointer(bitmap), rm_dev = refmap && is_device_pointer(refmap);
        const size_t o_pts = take(pts_dev ? 0 : npoints * ffi_affine_sz), o_bm = take(bm_dev ? 0 : nwords * 4),
                     o_rm = take(refmap && !rm_dev ? nwords * 4 : 0), o_conv = take(INTERNAL ? npoints * conv_stride() : 0),
                     o_keyA = take(nrec * 4), o_ptA = take(nrec * sizeof(bucket_t)),
                     o_keyB = take((nrec / F + 2) * 2 * 4), o_ptB = take((nrec / F + 2) * 2 * sizeof(bucket_t)),
                     o_bucket = take(sizeof(bucket_t)), o_fin = take(sizeof(std_bucket_t));
        reserve(o);
        reserve_sums(1);
        const unsigned char* d_points = (const unsigned char*)points;
        const u32 *d_bm = bitmap, *d_rm = refmap;
        if (!pts_dev) { HIP_OK(hipMemcpyAsync(blob + o_pts, points, npoints * ffi_affine_sz, hipMemcpyHostToDevice, stream)); d_points = blob + o_pts; }
        if (!bm_dev) { HIP_OK(hipMemcpyAsync(blob + o_bm, bitmap, nwords * 4, hipMemcpyHostToDevice, stream)); d_bm = (const u32*)(blob + o_bm); }
        if (refmap && !rm_dev) { HIP_OK(hipMemcpyAsync(blob + o_rm, refmap, nwords * 4, hipMemcpyHostToDevice, stream)); d_rm = (const u32*)(blob + o_rm); }
        const bool flagged = ffi_affine_sz > 2 * FP_BYTES;
        if constexpr (INTERNAL) {
            launch_convert(blob + o_conv, d_points, (unsigned)npoints, ffi_affine_sz);
            d_points = blob + o_conv;
        }
        bucket_t* bucket = (bucket_t*)(blob + o_bucket);
        HIP_OK(hipMemsetAsync(bucket, 0, sizeof(bucket_t), stream));
        u32* ik = (u32*)(blob + o_keyA); bucket_t* ip = (bucket_t*)(blob + o_ptA);
        u32* ok = (u32*)(blob + o_keyB); bucket_t* op = (bucket_t*)(blob + o_ptB);
        {
            dim3 grid((unsigned)((nrec + 255) / 256));
            if (flagged) hipLaunchKernelGGL((k_bitmap_accumulate<fp_d, true>), grid, dim3(256), 0, stream, ik, ip, d_points,
                                            (unsigned)ffi_affine_sz, (unsigned)npoints, d_bm, d_rm, span);
            else         hipLaunchKernelGGL((k_bitmap_accumulate<fp_d, false>), grid, dim3(256), 0, stream, ik, ip, d_points,
                                            (unsigned)ffi_affine_sz, (unsigned)npoints, d_bm, d_rm, span);
            HIP_OK(hipGetLastError());
        }
        for (size_t n = nrec;;) {                                   // the MSM's record tree, every key = 0
            unsigned nthreads = (unsigned)((n + F - 1) / F);
            int last = nthreads == 1;
            hipLaunchKernelGGL(k_reduce_runs<fp_d>, dim3((nthreads + 255) / 256), dim3(256), 0, stream,
                               bucket, ok, op, ik, ip, (unsigned)n, (unsigned)F, nthreads, last, (const u32*)nullptr);
            HIP_OK(hipGetLastError());
            if (last) break;
            n = (size_t)2 * nthreads;
            std::swap(ik, ok); std::swap(ip, op);
        }
        if constexpr (INTERNAL) {
            std_bucket_t* fin = (std_bucket_t*)(blob + o_fin);
            hipLaunchKernelGGL((k_finalize<fp_d, STD_WORDS>), dim3(1), dim3(64), 0, stream, fin, bucket, 1u);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(h_sums, fin, sizeof(std_bucket_t), hipMemcpyDeviceToHost, stream));
        } else {
            HIP_OK(hipMemcpyAsync(h_sums, bucket, sizeof(std_bucket_t), hipMemcpyDeviceToHost, stream));
        }
        HIP_OK(hipStreamSynchronize(stream));
        fp_h c[4];
        memcpy(c, h_sums, sizeof(c));
        out = point_t::from_xyzz(c[0], c[1], c[2], c[3]);
    }

    // out: Jacobian X|Y|Z (Montgomery).  points: stride ffi_affine_sz, flagged
    // format iff ffi_affine_sz > 2*FP_BYTES.  scalars: SCALAR_BYTES each.
    void invoke(point_t& out, const void* points, size_t npoints, const void* scalars,
                bool mont, size_t ffi_affine_sz)
    {   invoke_form(out, points, npoints, scalars, mont, ffi_affine_sz, scalar_form());   }

    // The same over SHORT scalars (include/sppark_amd_short.h): plain integers of |bits| significant bits, |stride| bytes
    // apart; the result is the MSM of s_i mod 2^bits.  Refused (hipErrorInvalidValue) outside the contract, before the
    // device is selected or a byte is read.  On a context with fixed-base tables the call runs the ordinary path over the
    // preloaded points themselves (level 0 of the table), as a call of any other length does.
    void invoke_short(point_t& out, const void* points, size_t npoints, const void* scalars,
                      unsigned bits, size_t stride, size_t ffi_affine_sz)
    {
        out.set_inf();
        check_short(bits, stride, scalars);
        invoke_form(out, points, npoints, scalars, false, ffi_affine_sz, scalar_form(bits, stride));
    }

private:
    void invoke_form(point_t& out, const void* points, size_t npoints, const void* scalars,
                     bool mont, size_t ffi_affine_sz, const scalar_form& sf)
    {
        out.set_inf();
        if (npoints == 0) return;
        if (npoints > (1u << 31)) HIP_OK(hipErrorInvalidValue);
        HIP_OK(hipSetDevice(gpu->hip_id));
        const bool preconverted = INTERNAL && points == nullptr;      // preload() already converted them
        if (points == nullptr) {                    // preloaded points, their own stride
            if (npoints > pre_n) HIP_OK(hipErrorInvalidValue);
            points = pre_points; ffi_affine_sz = pre_stride;
        }
        if (scalars == nullptr || ffi_affine_sz < 2 * FP_BYTES) HIP_OK(hipErrorInvalidValue);
        join_default_stream();
        // fixed-base tables cover exactly the preloaded vector: any other length runs the ordinary path on its first level
        if (preconverted && pre_fb_nwins && sf.bits == 0 && npoints == pre_n && tune.chunk == 0 && tune.max_scratch == 0 && fixed_fits(npoints, scalars)) {
            invoke_fixed(out, npoints, scalars, mont);
            return;
        }

        const bool pts_dev = is_device_pointer(points), sc_dev = is_device_pointer(scalars);
        const bool host = !pts_dev || !sc_dev;
        const size_t chunk = choose_chunk(npoints, (pts_dev ? 0 : ffi_affine_sz) + (sc_dev ? 0 : sf.stride), sf.plan_bits());
        const std::vector<size_t> cb = chunk_bounds(npoints, chunk);
        const size_t nchunks = cb.size() - 1;
        const size_t in_stride = preconverted ? conv_stride() : ffi_affine_sz;     // bytes between input records
        if (nchunks > 4096) HIP_OK(hipErrorOutOfMemory);

        // one plan (and layout) per chunk; scratch for the largest
        std::vector<msm_plan> plans(nchunks);
        std::vector<layout> layouts(nchunks);
        size_t need = 0, longest = 0;
        for (size_t c = 0; c < nchunks; c++) {
            plans[c] = make_plan(cb[c + 1] - cb[c], sf.plan_bits(), tune);
            if (plans[c].nwins > MAX_WINS) HIP_OK(hipErrorInvalidValue);
            layouts[c] = make_layout(plans[c], !preconverted);
            need = std::max(need, layouts[c].total); longest = std::max(longest, cb[c + 1] - cb[c]);
        }
        reserve(need);
        reserve_sums(nchunks * MAX_WINS + 1);                    // (+ the small sizes' flag word behind the sums of a one-chunk MSM)
        const size_t st_pts = align_up(pts_dev ? 0 : longest * ffi_affine_sz), st_sc = align_up(sc_dev ? 0 : longest * sf.stride);
        if (host) { reserve_stage(2 * (st_pts + st_sc)); if (nchunks > 1) need_cpy(); }

        for (size_t c = 0; c < nchunks; c++) {
            const size_t lo = cb[c], cn = cb[c + 1] - lo;
            const msm_plan& p = plans[c];
            const layout& l = layouts[c];
            const unsigned sb = c & 1;
            const unsigned char* d_points = (const unsigned char*)points + lo * in_stride;
            const u32* d_scalars = (const u32*)((const unsigned char*)scalars + lo * sf.stride);
            if (host) {
                // copies of chunk c: scalars first (the sort only needs them).  With more than one chunk they run
                // on the copy stream, under the arithmetic of chunk c-1; pageable source memory makes the call
                // itself block until the data has left the host buffer, which is fine: chunk c-1's kernels are
                // already queued.
                hipStream_t cs = nchunks > 1 ? cpy : stream;
                unsigned char* sp = stage + sb * (st_pts + st_sc);
                if (nchunks > 1 && c >= 2) HIP_OK(hipStreamWaitEvent(cpy, ev_chunkdone[sb], 0));    // chunk c-2 is done with this set
                if (!sc_dev) {
                    HIP_OK(hipMemcpyAsync(sp + st_pts, d_scalars, cn * sf.stride, hipMemcpyHostToDevice, cs));
                    d_scalars = (const u32*)(sp + st_pts);
                }
                if (!pts_dev) {
                    HIP_OK(hipMemcpyAsync(sp, d_points, cn * ffi_affine_sz, hipMemcpyHostToDevice, cs));
                    d_points = sp;
                }
                if (nchunks > 1) {
                    HIP_OK(hipEventRecord(ev_copied[sb], cpy));
                    HIP_OK(hipStreamWaitEvent(stream, ev_copied[sb], 0));
                }
            }
            // (chunks of different lengths have layouts of their own: harmless, every sort set of an MSM is
            // either written on the main stream or behind an event recorded on it after the previous MSM)
            enqueue(p, l, d_points, in_stride, preconverted, d_scalars, mont, h_sums + c * MAX_WINS, c == 0, 0, 0, false, nchunks == 1, sf);
            if (host && nchunks > 1) HIP_OK(hipEventRecord(ev_chunkdone[sb], stream));
        }
        HIP_OK(hipStreamSynchronize(stream));
        last_chunks = (unsigned)nchunks;
        // the piece tree left a bucket with more pieces than it takes (skewed scalars): the fan-in tree over the records it
        // left, the bucket sums again (single chunk: the piece tree is for sizes far below a chunk)
        if (piece_pending && *h_flag_cur != 0) {
            enqueue(plans[0], layouts[0], nullptr, in_stride, preconverted, nullptr, mont, h_sums, false, 0, 0, true, false, sf);
            HIP_OK(hipStreamSynchronize(stream));
            last_redo++;
        }
        piece_pending = false;

        if (timing) {
            const msm_plan& p = plans[0];
            float acc = 0, t;
            for (unsigned g = 0; g < p.G; g++) { HIP_OK(hipEventElapsedTime(&t, tev[2 + 2 * g], tev[3 + 2 * g])); acc += t; }
            HIP_OK(hipEventElapsedTime(&last_ms[0], tev[0], tev[2]));
            last_ms[1] = acc;
            HIP_OK(hipEventElapsedTime(&last_ms[2], tev[0], tev[1]));
            last_ms[3] = (float)p.G;
        }

        for (size_t c = 0; c < nchunks; c++) {
            point_t part = horner(h_sums + c * MAX_WINS, plans[c]);
            out.add(part);
        }
    }
};

} // namespace sppark_amd
