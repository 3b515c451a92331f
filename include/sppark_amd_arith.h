/*
 * sppark_amd field-vector arithmetic, polynomial product and vanishing quotient: what sits BETWEEN two transforms of
 * a prover -- the sum, difference and product of two field vectors that live on the device -- and the two everyday
 * compositions of it with compute_ntt.  The reference has no counterpart; its callers write these loops themselves.
 *
 * Elements are in the wire format of compute_ntt (sppark_amd.h, section 3) and must be canonical (every component
 * below the modulus); outputs are canonical, so a result is one bit pattern.
 *
 * Pointwise, declared in every product library over the library's field (libsppark_gl64, _gl64_plonky2, _bb31,
 * _bb31_canonical, the five curve libraries over the curve's scalar field Fr, libsppark_m31, libsppark_bb31x4):
 *
 *   sppark_field_add     out[i] = a[i] + b[i]
 *   sppark_field_sub     out[i] = a[i] - b[i]
 *   sppark_field_mul     out[i] = a[i] * b[i]
 *   sppark_field_scale   out[i] = a[i] * k[0]
 *   sppark_field_mul_sub out[i] = (a[i] * b[i] - c[i]) * k[0]; k == NULL: one, and no product is spent on it
 *
 * out may be identical to any input and inputs may be identical to each other (a == b: a square); any two buffers
 * must be identical or disjoint.  Any element-aligned pointer works; 16-byte aligned ones run with 16-byte accesses.
 * k is ONE element, on the host (passed to the kernel by value) or on the device (read there); it may not lie
 * inside out.  Pointers may be host or device pointers; host buffers are staged through the device.
 *
 * Streams: when EVERY buffer is a device pointer and the stream is not NULL the call only enqueues its one launch
 * -- no allocation, no copy, no synchronisation: it can be captured into a graph -- as sppark_ntt_batch does.  Every
 * other call returns when the result is in place.
 *
 * len == 0 succeeds and touches nothing.  Rejected before a device is looked up (negated hipErrorInvalidValue, owned
 * message): a NULL buffer with len > 0, len * sizeof(element) overflowing size_t, two buffers that overlap partially.
 *
 * Declared in the nine libraries that have compute_ntt (not in libsppark_m31 / libsppark_bb31x4):
 *
 *   sppark_poly_product: out[0 .. la+lb-1) = the coefficients of (sum a_i x^i)(sum b_i x^i), lowest first.  la == 0
 *     or lb == 0 succeeds and touches nothing.  out must be disjoint from a and b; a and b may overlap freely (a == b
 *     with la == lb: a square, one forward transform).  With n = 2^lg the least power of two >= la+lb-1, lg above the
 *     field's 2-adicity is rejected before a device is looked up.  Device scratch: 2n elements from the library's
 *     pool.  One padding launch, ONE forward transform of both columns, the pointwise product, one inverse transform,
 *     no bit reversal anywhere.  The call returns when the result is in place.
 *
 *   sppark_poly_vanishing_quotient: a, b, c hold n = 2^lg_domain_size evaluations over {w^i} in natural order; h
 *     receives the n coefficients, lowest first, of what these public calls give:
 *       compute_ntt(NN, Inverse, Standard) on each of a, b, c;  compute_ntt(NN, Forward, Coset) on each;
 *       t = (a .* b - c) * k with k = 1 / (g^n - 1), g the generator of the Coset type;  h = compute_ntt(NN, Inverse, Coset)(t)
 *     When c[i] = a[i] * b[i] for every i (a satisfied R1CS) that is the exact quotient of A*B - C by x^n - 1 --
 *     Groth16's h -- with h[n-1] == 0, whatever g is.  The inputs are not modified; h may be identical to one of them
 *     or disjoint from all.  lg_domain_size above the 2-adicity is rejected before a device is looked up.  Device
 *     scratch: 3n elements.  The call returns when the result is in place.
 */
#ifndef SPPARK_AMD_ARITH_H
#define SPPARK_AMD_ARITH_H

#include "sppark_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_field_add(size_t device_id, void *out, const void *a, const void *b, size_t len, void *stream);
SppError sppark_field_sub(size_t device_id, void *out, const void *a, const void *b, size_t len, void *stream);
SppError sppark_field_mul(size_t device_id, void *out, const void *a, const void *b, size_t len, void *stream);
SppError sppark_field_scale(size_t device_id, void *out, const void *a, const void *k, size_t len, void *stream);
SppError sppark_field_mul_sub(size_t device_id, void *out, const void *a, const void *b, const void *c,
                              const void *k /* NULL: one */, size_t len, void *stream);

SppError sppark_poly_product(size_t device_id, void *out, const void *a, size_t la, const void *b, size_t lb, void *stream);
SppError sppark_poly_vanishing_quotient(size_t device_id, void *h, const void *a, const void *b, const void *c,
                                        uint32_t lg_domain_size, void *stream);

#ifdef __cplusplus
}
#endif
#endif
