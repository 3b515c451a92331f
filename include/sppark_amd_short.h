/*
 * sppark_amd MSM over SHORT scalars: the caller declares how many bits its scalars have, and only the windows of
 * those bits are sorted, accumulated and summed.  The reference's CPU Pippenger takes the bit length
 * (msm/pippenger.hpp:83-89,225); its GPU path, like the entry points of sppark_amd.h, always runs the full width of
 * the scalar field.
 *
 * Who has such scalars: commitments to witness / trace columns of 64-bit, 32-bit or byte values, 128-bit challenges
 * of batched verification, the short half of a GLV split.  With the calls below they are passed as they are -- no
 * zero-extension to 32 bytes -- and a 2^26-point MSM over 64-bit scalars runs 3 windows of 22 bits instead of 12.
 *
 * Declared in the five curve libraries (libsppark_bls12_381, _bn254, _bls12_377, _pallas, _vesta; the G2 one-shot
 * where the curve has a G2).
 *
 * CONTRACT.  scalar_bits = b, scalar_stride = S:
 *   - 1 <= b <= NBITS - 2, NBITS the bit length of the scalar field's modulus (255 for BLS12-381, 254 for alt_bn128,
 *     253 for BLS12-377, 255 for the Pasta curves).  Full-width scalars keep using the entry points of sppark_amd.h.
 *   - S = bytes between consecutive scalars: a multiple of 4 with 4 * ceil(b / 32) <= S <= 32.
 *   - the scalars' base address is S-aligned for S = 4, 8, 16 and 4-aligned otherwise.  Host or device pointer.
 *   - a scalar is a little-endian unsigned integer in PLAIN form (there is no Montgomery flag on these calls).
 *   - THE VALUE USED IS THE LOW b BITS.  The kernel reads only the ceil(b / 32) words that hold them and masks the
 *     top one; bits from b up to 8 * S are never looked at.  The result is therefore always
 *         sum_i (s_i mod 2^b) * P_i,
 *     deterministically, whether or not the caller's scalars were below 2^b (short values may sit in wider slots with
 *     anything above them).
 *   - a call outside this range -- b == 0, b > NBITS - 2, a stride that is too small for b, above 32 or no multiple
 *     of 4, a misaligned base -- is refused with the negated hipErrorInvalidValue and an owned message BEFORE any
 *     memory is touched and before a device is looked up; *out is the point at infinity.
 *
 * PLAN.  The windows are those of make_plan(npoints, b + 1): the extra bit is zero in every scalar, so the signed
 * digit of the top window never carries out (the full-width path gets the same from folding s > r/2 to r - s; here no
 * fold is needed).  sppark_msm_plan_bits reports that plan in the layout of sppark_msm_plan.
 *
 * FIXED-BASE TABLES.  On a context whose points were set with sppark_msm_set_points_fixed_base a short call runs the
 * ordinary path over the preloaded points themselves -- what a call of any other length than the tables' does.
 *
 * Window groups, the chunked host path, preloaded bases (points == NULL), host / device pointers in any mix: as
 * sppark_msm_invoke.  The one-shot calls follow mult_pippenger_inf / mult_pippenger_fp2_inf (pooled context,
 * synchronous, Affine_inf_t points of stride ffi_affine_sz).
 */
#ifndef SPPARK_AMD_SHORT_H
#define SPPARK_AMD_SHORT_H

#include "sppark_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* points == NULL: the preloaded bases */
SppError sppark_msm_invoke_bits(sppark_msm_ctx *ctx, void *out, const void *points, size_t npoints,
                                const void *scalars, unsigned scalar_bits, size_t scalar_stride,
                                size_t ffi_affine_sz);
/* sppark_msm_reserve for calls of this scalar form */
SppError sppark_msm_reserve_bits(sppark_msm_ctx *ctx, size_t npoints, size_t ffi_affine_sz,
                                 int host_points, int host_scalars,
                                 unsigned scalar_bits, size_t scalar_stride);
/* the layout of sppark_msm_plan; scalar_bits outside 1 .. NBITS - 2: all zero */
void     sppark_msm_plan_bits(const sppark_msm_ctx *ctx, size_t npoints, unsigned scalar_bits,
                              unsigned out[8]);
/* one-shot, pooled context, synchronous */
SppError mult_pippenger_inf_bits(void *out, const void *points, size_t npoints, const void *scalars,
                                 unsigned scalar_bits, size_t scalar_stride, size_t ffi_affine_sz);
/* ... over G2 (not in the Pasta libraries) */
SppError mult_pippenger_fp2_inf_bits(void *out, const void *points, size_t npoints, const void *scalars,
                                     unsigned scalar_bits, size_t scalar_stride, size_t ffi_affine_sz);

#ifdef __cplusplus
}
#endif
#endif
