// HOST EMULATION TEST HARNESS (tests only): the products of ff/montx_dev.hpp -- operator*, mul2, mul_add, sqr2, sqr, whose
// columns are the generated blocks of ff/montx_blocks.hpp -- on raw limbs, for tests/test_montx_blocks.py.  The host pass
// compiles the #else body of every block (the plain C of the asm statement's steps); the caller compares limb for limb with
// a column-by-column model in Python.  which = 0: the curve's G1 bucket field (msm_fp_d), 1: the base field of its G2
// bucket field (fp2_d::fp: ten 28-bit limbs over alt_bn128).
#define SPPARK_HOST_EMULATION 1
#include "../../sppark_amd/csrc/msm/curve_select.hpp"

using namespace sppark_amd;

namespace {
template<class F> int info(int* out)
{
    out[0] = F::NL; out[1] = F::LIMB_BITS; out[2] = F::FAT_M_OK ? 1 : 0; out[3] = F::MA_A0; out[4] = F::MA_A1; out[5] = F::SQR_L;
    for (int j = 0; j < F::NL; j++) out[8 + j] = (int)F::mod_limb(j);
    return 0;
}
// form 0: a0 * b0          1: mul2(a0, b0, a1, b1)      2: mul2<true, true>      3: mul2<true, false>
//      4: mul_add          5: sqr2(a0, a1)              6: a0.sqr()
// r0 | r1: NL limbs each per element (r1 untouched by the single forms)
template<class F> int run(int form, u32* r0, u32* r1, const u32* a0, const u32* b0, const u32* a1, const u32* b1, size_t n)
{
    constexpr int NL = F::NL;
    for (size_t i = 0; i < n; i++) {
        F x0 = F::from_wire(a0 + i * NL), y0 = F::from_wire(b0 + i * NL), x1 = F::from_wire(a1 + i * NL), y1 = F::from_wire(b1 + i * NL);
        F p = F::zero(), q = F::zero();
        switch (form) {
            case 0: p = x0 * y0; break;
            case 1: F::mul2(p, q, x0, y0, x1, y1); break;
            case 2: F::template mul2<true, true>(p, q, x0, y0, x1, y1); break;
            case 3: F::template mul2<true, false>(p, q, x0, y0, x1, y1); break;
            case 4: p = F::mul_add(x0, y0, x1, y1); break;
            case 5: F::sqr2(p, q, x0, x1); break;
            case 6: p = x0.sqr(); break;
            default: return -1;
        }
        p.to_wire(r0 + i * NL); q.to_wire(r1 + i * NL);
    }
    return 0;
}
}

extern "C" int emu_blocks_info(int which, int* out)
{
    if (which == 0) return info<msm_fp_d>(out);
#ifndef SPPARK_NO_G2
    if (which == 1) return info<fp2_d::fp>(out);
#endif
    return -1;
}
extern "C" int emu_blocks_run(int which, int form, u32* r0, u32* r1, const u32* a0, const u32* b0, const u32* a1, const u32* b1, size_t n)
{
    if (which == 0) return run<msm_fp_d>(form, r0, r1, a0, b0, a1, b1, n);
#ifndef SPPARK_NO_G2
    if (which == 1) return run<fp2_d::fp>(form, r0, r1, a0, b0, a1, b1, n);
#endif
    return -1;
}
