/*
 * sppark_amd multilinear tables and sumcheck rounds: the inner loop of a sumcheck prover (Spartan, HyperPlonk, GKR,
 * Lasso / Jolt) on evaluation tables that live on the device.  The reference has no counterpart.
 *
 * A table f has n = 2^lg_n elements of the library's field in the wire format of compute_ntt (sppark_amd.h, section 3).
 * Elements are canonical in and canonical out, so every result is one bit pattern.  Index i = sum_j i_j 2^j, and variable j
 * is bit j.  The multilinear extension is
 *
 *   f~(x_0 .. x_{lg_n-1}) = sum_i f[i] * prod_j (i_j ? x_j : 1 - x_j)
 *
 * order names the variable a call binds and the pairs (lo_i, hi_i), i < n/2, it forms:
 *   SPPARK_MLE_LOW   variable 0:          (f[2i], f[2i+1])
 *   SPPARK_MLE_HIGH  variable lg_n - 1:   (f[i], f[i + n/2])
 *
 * sppark_mle_fold      out[i] = lo_i + r (hi_i - lo_i), n/2 elements.  r is ONE element, on the host (passed by value) or
 *   on the device (read there), as k of sppark_field_scale; it may not lie inside out.  lg_n == 0 is rejected.  HIGH: out
 *   may be identical to in (the first half is overwritten) or disjoint from all n elements of in.  LOW: out must be
 *   disjoint from in.  When every buffer is a device pointer and the stream is not NULL the call only enqueues its one
 *   launch -- no allocation, no copy, no synchronisation: it can be captured -- the sppark_field_* contract.
 *
 * sppark_mle_evaluate  ret[0] = f~(point[0] .. point[lg_n-1]).  point holds lg_n elements, on the host or the device; in is
 *   not modified (ret may not lie inside in or point).  lg_n == 0 gives ret[0] = in[0].  ceil(lg_n / T) launches, T = 12 /
 *   11 / 10 / 9 for elements of 4 / 8 / 16 / 32 bytes: one read of the table plus 2^-T of it for every later pass; scratch
 *   from the library's pool.  The call returns when the result is in place.
 *
 * sppark_mle_eq        out[i] = prod_j (i_j ? point[j] : 1 - point[j]), n elements; lg_n == 0 gives one element, the field's
 *   one.  One launch, one write of the table.  out may not overlap point.  The call returns when the result is in place.
 *
 * sppark_sumcheck_round  one round polynomial.  tables is a HOST array of ntables pointers, each to n elements; each pointer
 *   may be a host or a device pointer.  With f_k,i(t) = lo + t (hi - lo) for the pair i of table k,
 *   out[t] = s(t) for t = 0 .. d (d + 1 elements, host or device), t the field element 1 + .. + 1:
 *     SPPARK_SUMCHECK_PRODUCT     1 <= ntables <= 4, d = ntables:  s(t) = sum_i prod_k f_k,i(t)
 *     SPPARK_SUMCHECK_EQ_MUL_SUB  ntables == 4 in the order e, a, b, c, d = 3:  s(t) = sum_i e_i(t) (a_i(t) b_i(t) - c_i(t)),
 *                                 the zero-check of an R1CS, the sumcheck sibling of sppark_field_mul_sub
 *   Tables may be identical to each other (any two must be identical or disjoint); out must be disjoint from all.
 *   lg_n == 0 is rejected.  Two launches; the result does not depend on the grid.  The call returns when the result is in
 *   place.
 *
 * Common to all four: lg_n > 32 is rejected.  Rejected before a device is looked up (negated hipErrorInvalidValue, owned
 * message): NULL buffers, byte counts that overflow size_t, partial overlaps, an unknown order or form, a wrong ntables.
 * Host buffers are staged through the device.  Declared in every product library over the library's own field, libsppark_m31
 * and libsppark_bb31x4 included; a BabyBear prover that needs extension-field challenges lifts its table to bb31x4 itself.
 */
#ifndef SPPARK_AMD_MLE_H
#define SPPARK_AMD_MLE_H

#include "sppark_amd.h"

#define SPPARK_MLE_LOW 0
#define SPPARK_MLE_HIGH 1
#define SPPARK_SUMCHECK_PRODUCT 0
#define SPPARK_SUMCHECK_EQ_MUL_SUB 1

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_mle_fold(size_t device_id, void *out, const void *in, uint32_t lg_n, const void *r, int order, void *stream);
SppError sppark_mle_evaluate(size_t device_id, void *ret, const void *in, uint32_t lg_n, const void *point, void *stream);
SppError sppark_mle_eq(size_t device_id, void *out, const void *point, uint32_t lg_n, void *stream);
SppError sppark_sumcheck_round(size_t device_id, void *out, const void *const *tables, size_t ntables, int form, uint32_t lg_n,
                               int order, void *stream);

#ifdef __cplusplus
}
#endif
#endif
