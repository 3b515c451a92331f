/*
 * sppark_amd batched NTT / LDE: many polynomials of one size in one call.
 *
 * Declared in every library that has compute_ntt (libsppark_gl64, _bb31, _gl64_plonky2, _bb31_canonical and the five
 * curve libraries, over the curve's scalar field); not in libsppark_m31 / _bb31x4.  Elements as in sppark_amd.h.
 *
 * sppark_ntt_batch: |batch| in-place transforms of 2^lg_domain_size elements each.
 *   Column j is inout[j*stride .. j*stride + 2^lg).  |stride| is in elements: 0 means 2^lg, otherwise it must be at
 *   least 2^lg.  Elements between columns are never read or written.  Every column gets, bit for bit, what sppark_ntt
 *   gives it, in every order x direction x type.  (From 2^12 elements on, Goldilocks / BabyBear columns move 16 bytes
 *   per access, as sppark_ntt does: columns that start 16-byte aligned are the fast layout.)
 * sppark_lde_batch: |batch| low-degree extensions.  Column j owns inout[j*ext .. (j+1)*ext), ext = 2^(lg+lg_blowup);
 *   its first 2^lg elements hold the evaluations.  Each column's result equals sppark_lde's.  aux_out is NULL or holds
 *   batch x 2^lg packed elements: column j's coefficients go to aux_out + j*2^lg.
 *
 * No-ops: batch == 0 succeeds and does nothing, as does lg_domain_size == 0 for the NTT.  An LDE with
 * lg_domain_size == 0 behaves like sppark_lde on each column.
 * Rejected before anything is allocated, copied or launched (negated HIP code, owned message): lg (+ lg_blowup) above
 * the field's 2-adicity, an order outside 0..3, 0 < stride < 2^lg, byte extents that overflow size_t, and for a device
 * pointer an extent past the end of the allocation that holds inout or aux_out.
 * Streams as sppark_ntt / sppark_lde: sppark_ntt_batch on a device buffer with a non-NULL stream only enqueues the work;
 * everything else returns when the work is done.
 * Host buffers are staged through the device in chunks of whole columns; so is the LDE's device scratch (the coefficient
 * buffer, and a staged aux_out).  Device scratch per call: at most max(one column's need, SPPARK_BATCH_CHUNK_BYTES).
 *
 * How the columns run (DESIGN.md "Batched transforms"): every launch of the single-transform plan takes one grid row
 * per column (blockIdx.y) and all columns share the twiddle tables; columns of 2^1 ... 2^6 elements are packed several
 * to a wave instead (k_ntt_small_packed).  A batch above the device's grid limit is split into several launches;
 * sppark_ntt_batch_launch_cols says how many columns one launch covers.
 *
 * Measured on one MI355X (profiles/r07_ntt_batch.log; device buffers, non-NULL stream): a batch of 2^24 Goldilocks elements
 * takes 0.040 / 0.052 / 0.078 / 0.123 / 0.083 / 0.150 / 0.181 ms at columns of 2^2 / 2^5 / 2^8 / 2^11 / 2^12 / 2^16 / 2^20
 * (forward NR), against 0.213 ms for one 2^24 transform and 32.6 ms for the loop of 4096 sppark_ntt calls at 2^12 (394x);
 * BabyBear 0.025 ... 0.086 against 0.097; BLS12-381, 2^22 elements, 0.054 ... 0.507 against 0.569.  64 Goldilocks LDEs
 * 2^16 -> 2^18: 0.177 ms against 0.246 for one 2^22 -> 2^24 LDE.  Targets: a batch no slower than one transform of the
 * total size -- met at every column size up to 2^16, at parity (0.99 - 1.03x) for inverse and coset transforms of 2^20
 * columns; at least 10x the per-column loop at 2^12 -- met (59 - 488x); the LDE target -- met; single transforms
 * unchanged within the run-to-run spread.  DESIGN.md "Batched transforms" has the table and the reasons.
 */
#ifndef SPPARK_AMD_BATCH_H
#define SPPARK_AMD_BATCH_H

#include "sppark_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device scratch of one call (bytes) beyond which host columns and LDE scratch are processed in chunks */
#define SPPARK_BATCH_CHUNK_BYTES ((size_t)256 << 20)

SppError sppark_ntt_batch(size_t device_id, void *inout, uint32_t lg_domain_size, size_t batch, size_t stride,
                          int ntt_order, int ntt_direction, int ntt_type, void *stream);
SppError sppark_lde_batch(size_t device_id, void *inout, uint32_t lg_domain_size, uint32_t lg_blowup, size_t batch,
                          void *aux_out, void *stream);
/* columns of 2^lg_domain_size elements one launch of sppark_ntt_batch covers on this device (0: no device, or an lg the
 * field does not accept) */
size_t sppark_ntt_batch_launch_cols(size_t device_id, uint32_t lg_domain_size);

#ifdef __cplusplus
}
#endif
#endif
