// HOST EMULATION of k_ntt_small_packed, the batched NTT's kernel for columns of 2^1 ... 2^6 elements (tests only; see
// emu_ntt.cpp, whose harness this file reuses).  Every work-group of 256 lanes runs as 256 host threads, each calling the
// kernel's own lane function ntt_packed_lane (ntt_kernels.hpp) with (blockIdx.y, threadIdx.x): its column mapping, segment
// lanes, the partial last work-group and waves, and ntt_rx_run's exchanges through the emulated LDS buffers (on the GPU:
// permlane16_swap / DPP / ds_bpermute inside the segment).
#include "emu_ntt.cpp"

// the route of a batch of |batch| columns |stride| elements apart; returns 0 (nothing done) where it is not one launch of
// k_ntt_small_packed over all of them
extern "C" int emu_ntt_batch(void* inout, unsigned lg, size_t batch, size_t stride, int order, int direction, int type)
{
    if (lg == 0 || batch == 0) return 0;
    ntt_call c = emu_call(lg, order, direction, type);
    c.batch = batch; c.col_stride = stride;
    const ntt_route r = make_ntt_route(g_field, g_knobs, c);
    if (r.invalid || r.nsteps != 1 || r.steps[0].kernel != NK_SMALL_PACKED || r.cols != batch) return 0;
    emu_run_route(r, (F*)inout, lg, 256, emu_lde_io{}, batch, stride);
    return 1;                                                   // (the packed kernel ran)
}
