// HOST EMULATION of k_ntt_small_packed, the batched NTT's kernel for columns of 2^1 ... 2^6 elements (tests only; see
// emu_ntt.cpp, whose harness this file reuses).  Every work-group of 256 lanes runs as 256 host threads, each calling the
// kernel's own lane function ntt_packed_lane (ntt_kernels.hpp) with (blockIdx.y, threadIdx.x): its column mapping, segment
// lanes, the partial last work-group and waves, and ntt_rx_run's exchanges through the emulated LDS buffers (on the GPU:
// permlane16_swap / DPP / ds_bpermute inside the segment).
#include "emu_ntt.cpp"

// as ntt_engine::run() for a batch of |batch| columns |stride| elements apart at the packed sizes; returns 0 (nothing done)
// where the engine would not launch k_ntt_small_packed
extern "C" int emu_ntt_batch(void* inout, unsigned lg, size_t batch, size_t stride, int order, int direction, int type)
{
    if (lg == 0 || batch == 0) return 0;
    F* d = (F*)inout;
    if (!(batch > 1 && lg <= NTT_PACKED_MAX_LG && lg <= g_small_max)) return 0;      // (ntt_engine::run: not the packed kernel)
    const int inverse = direction == 1;
    unsigned h = lg;
    std::vector<F> lo(1u << h), hi(1), glo(1u << h), ghi(1), inner(ntt_inner_entries<F>::value);
    F w = top_root();
    for (unsigned k = F::TWO_ADICITY; k > lg; k--) w = w * w;
    F g = group_gen();
    if (inverse) { w = finv(w); g = finv(g); }
    for (size_t k = 0; k < std::max<size_t>(lo.size(), inner.size()); k++) {
        table_item(lo.data(), hi.data(), inner.data(), w, lg, h, k);
        table_item(glo.data(), ghi.data(), (F*)nullptr, g, lg, h, k);
    }
    F two = F::one() + F::one();
    ntt_tables<F> T{lo.data(), hi.data(), inner.data(), lg, h, finv(field_pow(two, lg))}, G{glo.data(), ghi.data(), nullptr, lg, h, F::one()};
    const unsigned flags = ntt_small_flags(order, inverse != 0, type == 1);
    const unsigned nh = 1u << (lg - 1), cpw = 256u / nh;
    const size_t groups = (batch + cpw - 1) / cpw;
    std::vector<F> lds(2 * 256 + 1);
    for (size_t y = 0; y < groups; y++) {                       // blockIdx.y: the kernel's own lane function, lanes as host threads
        run_group(256, [&](unsigned tid) {
            auto lane = [&](auto LG) {
                constexpr unsigned L = decltype(LG)::value;
                if (inverse) ntt_packed_lane<F, true, L>(d, lds.data(), T, G, flags, stride, batch, y, tid);
                else         ntt_packed_lane<F, false, L>(d, lds.data(), T, G, flags, stride, batch, y, tid);
            };
            switch (lg) {
                case 1: lane(std::integral_constant<unsigned, 1>()); break;
                case 2: lane(std::integral_constant<unsigned, 2>()); break;
                case 3: lane(std::integral_constant<unsigned, 3>()); break;
                case 4: lane(std::integral_constant<unsigned, 4>()); break;
                case 5: lane(std::integral_constant<unsigned, 5>()); break;
                default: lane(std::integral_constant<unsigned, 6>()); break;
            }
        });
    }
    return 1;                                                   // (the packed kernel ran)
}
