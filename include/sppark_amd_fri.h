/*
 * sppark_amd FRI: what a STARK prover runs between "the trace is committed" (sppark_merkle_commit) and "the queries are
 * opened" (sppark_merkle_open), on vectors that live on the device.  The reference has no counterpart.
 *
 *   sppark_fri_reduce   the DEEP combination: one weighted sum over the columns of the committed matrix
 *   sppark_fri_domain   the points of the evaluation domain, less a constant: the denominators x_i - z
 *   sppark_fri_fold     one to three FRI folds of a codeword in one launch
 *
 * Elements are in the wire format of compute_ntt (sppark_amd.h, section 3), canonical in and canonical out, so every result
 * is one bit pattern.
 *
 * Domain (fold and domain).  n = 2^lg_n.  w is the library's own root of order n, top_root^(2^(TWO_ADICITY - lg_n)): the
 * root compute_ntt uses, so what compute_ntt, sppark_ntt_batch and sppark_lde leave lies on this domain.  shift is ONE
 * element of the domain's field in wire form ON THE HOST; NULL means 1; zero (and, in the single-word fields, a word that is not canonical) is rejected.  The
 * library's group generator is the coset of compute_ntt's Coset type and of sppark_lde's output.
 *   SPPARK_FRI_NATURAL  index i holds x_i = shift * w^i                   (sppark_lde, order NN)
 *   SPPARK_FRI_BITREV   index i holds x_i = shift * w^bitrev_lg_n(i)      (order NR)
 * libsppark_bb31x4 has no transform of its own: its domain is that of libsppark_bb31 (default build) -- shift and the points
 * are bb31 elements of 4 bytes, values and challenges bb31x4.  lg_n above the field's 2-adicity, or above 32, is rejected.
 *
 * sppark_fri_fold(device_id, out, in, lg_n, lg_arity, beta, shift, order, stream)
 *   lg_arity == 1: in holds the n evaluations of f(x) = f_e(x^2) + x f_o(x^2); out receives the n/2 evaluations of
 *   f_e + beta f_o on the squared domain (shift^2, w^2) in the same order:
 *       out = (lo + hi) / 2 + beta (lo - hi) / (2 x)
 *   with the pairs (lo, hi) = (in[2k], in[2k+1]) in BITREV and (in[k], in[k + n/2]) in NATURAL, x the point of lo.  The
 *   folded polynomial has the coefficients c[2k] + beta c[2k+1] EXACTLY.  lg_arity = a in 1 .. 3 is by definition a single
 *   folds with beta, beta^2, beta^4: n / 2^a elements, bit for bit those of the single folds, in ONE launch that reads every
 *   input once (a lane holds the 2^a inputs of a group: contiguous in BITREV, n / 2^a apart in NATURAL).
 *   beta is ONE element of the library's field, by host pointer (passed by value) or device pointer (read there), as r of
 *   sppark_mle_fold.  NATURAL: out may be identical to in (its first n / 2^a elements are overwritten) or disjoint from all
 *   of in.  BITREV: out must be disjoint from in.  Rejected: partial overlaps, beta inside out, lg_n < lg_arity, lg_arity
 *   outside 1 .. 3, an unknown order.  The twiddles 1 / (2 x) are never read from memory: a lane keeps the part that belongs
 *   to its place in a tile for the whole launch, and the part that belongs to the tile advances by one product per step.
 *
 * sppark_fri_domain(device_id, out, lg_n, shift, order, z, stream)
 *   out[i] = x_i - z as an element of the library's field (libsppark_bb31x4: the point in component 0); z is NULL (zero) or
 *   one element, host or device, and may not lie inside out.  One launch, one write of the vector.
 *
 * sppark_fri_reduce(device_id, out, in, in_base, lg_n, width, col_stride, leaf_stride, weights, sub, accumulate, stream)
 *   out[i] = (accumulate ? out[i] : 0) + sum_j weights[j] * e(j, i) - sub        for the n = 2^lg_n leaves i
 *   over the matrix of sppark_merkle_commit (sppark_amd_merkle.h): e(j, i) = in[j * col_stride + i * leaf_stride], columns
 *   layout (leaf_stride == 1, col_stride >= n) or rows layout (col_stride == 1, leaf_stride >= width), strides in elements of
 *   the matrix; bytes in the gaps of a stride are never read.  weights holds width elements of the library's field, on the
 *   host or the device -- a prover passes scale * alpha^j, so a power sequence continues over several matrices with
 *   accumulate.  sub is NULL or one element (host or device): the combination of the claimed openings.
 *   in_base == 1, in libsppark_bb31x4 only: the matrix holds bb31 elements (4 bytes, strides counted in those); weights, sub
 *   and out are bb31x4.  The committed BabyBear trace is combined under an extension-field challenge without being lifted.
 *   in_base == 1 is rejected in every other library.  Rejected as well: out overlapping in, weights or sub; width == 0; a size
 *   that overflows size_t; neither layout; lg_n > 32.
 *
 * Common to all three: when every buffer is a device pointer and the stream is not NULL the call only enqueues its one
 * launch -- no allocation, no copy, no synchronisation: it can be captured -- the sppark_field_* contract.  Host buffers are
 * staged through the device and the call returns when the result is in place.  Rejections come before a device is looked up
 * (negated hipErrorInvalidValue, owned message).
 *
 * sppark_fri_reduce is declared in every product library; sppark_fri_fold and sppark_fri_domain in every one with a 2-adic
 * domain, that is all but libsppark_m31 (the circle fold needs an extension of Mersenne31 that this library does not have).
 */
#ifndef SPPARK_AMD_FRI_H
#define SPPARK_AMD_FRI_H

#include "sppark_amd.h"

#define SPPARK_FRI_NATURAL 0
#define SPPARK_FRI_BITREV 1

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_fri_fold(size_t device_id, void *out, const void *in, uint32_t lg_n, uint32_t lg_arity, const void *beta,
                         const void *shift, int order, void *stream);
SppError sppark_fri_domain(size_t device_id, void *out, uint32_t lg_n, const void *shift, int order, const void *z, void *stream);
SppError sppark_fri_reduce(size_t device_id, void *out, const void *in, int in_base, uint32_t lg_n, size_t width, size_t col_stride,
                           size_t leaf_stride, const void *weights, const void *sub, int accumulate, void *stream);

#ifdef __cplusplus
}
#endif
#endif
