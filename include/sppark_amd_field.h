/*
 * sppark_amd field-vector inverse and quotient: the role of the reference's ff/batch_inversion.hpp (Montgomery's
 * trick: many inverses for one field inversion, zero mapped to zero) on a whole array that may live on the device.
 *
 * Declared in every product library, over the library's field: libsppark_gl64, _gl64_plonky2, _bb31, _bb31_canonical,
 * the five curve libraries (over the curve's scalar field Fr), libsppark_m31 and libsppark_bb31x4 (the quartic
 * extension: elements of four words).
 *
 * Elements are in the wire format of compute_ntt (sppark_amd.h, section 3) and must be canonical (every component
 * below the modulus); outputs are canonical, so a result is one bit pattern.
 *
 * sppark_field_inverse: out[i] = 1 / inp[i], and 0 where inp[i] == 0.  out == inp is allowed.
 * sppark_field_divide : out[i] = num[i] / den[i], and 0 where den[i] == 0.  out may equal num or den (or both).
 *
 * Pointers may be host or device pointers; host buffers are staged through the device like those of sppark_prefix_op.
 * Streams as sppark_prefix_op: the call returns when the result is in place.  len == 0 succeeds and touches nothing.
 * Rejected before a device is looked up (negated hipErrorInvalidValue, owned message): a NULL buffer with len > 0,
 * len * sizeof(element) overflowing size_t, and two buffers that overlap partially -- any two must be identical or
 * disjoint.
 *
 * How it runs (DESIGN.md "Field-vector inverse"): three launches -- tile products, one work-group that inverts them
 * with the call's single field inversion, and a pass that turns each tile's inverse into the inverses of its
 * elements through a product tree in LDS -- about 4 field products per element (5 for the quotient), two reads and
 * one write of the array.
 */
#ifndef SPPARK_AMD_FIELD_H
#define SPPARK_AMD_FIELD_H

#include "sppark_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_field_inverse(size_t device_id, void *out, const void *inp, size_t len, void *stream);
SppError sppark_field_divide(size_t device_id, void *out, const void *num, const void *den, size_t len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
