/*
 * sppark_amd Merkle commitments: the step between the transforms (sppark_ntt_batch, sppark_lde_batch, sppark_circle_lde) and
 * the queries of a STARK / FRI prover, on the matrix where the transforms left it.  The reference's snapshot has no
 * counterpart (its README names hash/ and merkle/).
 *
 * Matrix.  Element (j, i) is column j of leaf i, 0 <= j < width, 0 <= i < n = 2^lg_n, at
 *   in + (j * col_stride + i * leaf_stride) * sizeof(element)
 * with the library's field element (4, 8, 16 or 32 bytes).  Exactly two layouts are accepted:
 *   columns  leaf_stride == 1, col_stride >= n      one polynomial per row of a 2-D array, as the batched transforms leave
 *                                                   it: a leaf is a column of that array, nothing needs transposing
 *   rows     col_stride == 1, leaf_stride >= width  one leaf per row
 * Bytes in the gaps of a stride are never read.  in is aligned to the element, 16 bytes at the most.
 *
 * Leaf digest i = H(e(0,i) || e(1,i) || .. || e(width-1,i)): every element contributes its sizeof(element) bytes exactly as
 * stored, which is the wire format of compute_ntt (sppark_amd.h, section 3).  Every field value has one bit pattern there,
 * and the library's own outputs are canonical, so the commitment is well defined; a verifier hashes the same wire bytes.
 * Wire formats in Montgomery form: libsppark_bls12_381, bn254, bls12_377, pallas, vesta (R = 2^256) and libsppark_bb31,
 * bb31_canonical, bb31x4 (R = 2^32).  Plain canonical integers: libsppark_gl64, gl64_plonky2 and m31.  A verifier of a
 * Montgomery library's commitment hashes Montgomery bytes (canonical-integer serialisation is not offered).
 *
 * Node digest = H(left || right), 64 bytes.  H is unkeyed BLAKE2s-256 (RFC 7693; no salt, no personalisation) or SHA-256
 * (FIPS 180-4) with their standard padding: bit for bit Python's hashlib.blake2s(m).digest() / hashlib.sha256(m).digest().
 * Digests are stored as the standard byte strings.  The tree is a plain binary tree: no domain-separation bytes, no caps, no
 * mixed heights.  lg_n == 0: one leaf, whose digest is the root.
 *
 * Tree.  2^(lg_n+1) - 1 digests of 32 bytes.  Layer l (0 = leaves .. lg_n = root) holds 2^(lg_n-l) digests and starts at
 * digest index 2^(lg_n+1) - 2^(lg_n-l+1): the layers lie bottom-up, the root is the last 32 bytes.
 *
 * sppark_merkle_commit  tree: required, 16-byte aligned, SPPARK_MERKLE_TREE_BYTES(lg_n) bytes, host or device.  root: NULL,
 *   or 32 bytes, host or device, outside tree.  With in and tree on the device, root NULL or on the device, and a stream
 *   that is not NULL the call only enqueues its launches -- no allocation, no copy, no synchronisation: it can be captured
 *   -- the sppark_field_* contract.  Otherwise host buffers are staged through the device and the call returns when the
 *   results are in place.  Two launches up to lg_n = 10, 2 + ceil((lg_n - 10) / 3) above.
 *
 * sppark_merkle_open    paths[q][l] = the layer-l digest at index (indices[q] >> l) ^ 1, l = 0 .. lg_n - 1: nidx * lg_n * 32
 *   bytes, host or device, 16-byte aligned like tree.  indices is a HOST array (query indices come from a host transcript):
 *   every index is checked before a device is touched, and nothing is written when one is refused.  One gather launch.
 *   lg_n == 0 writes nothing.  The call returns when the paths are in place.
 *
 * sppark_merkle_gather  rows[q][j] = e(j, indices[q]): nidx * width elements, contiguous per query, host or device -- the
 *   opened row that travels with a path.  The same index rules; one launch.
 *
 * Rejected before a device is looked up (negated hipErrorInvalidValue, owned message): NULL tree / in / paths / rows; NULL
 * indices with nidx > 0; lg_n > SPPARK_MERKLE_MAX_LG; width == 0; width * sizeof(element) >= 2^32; a stride pair that is
 * neither layout; a size that overflows size_t; an unknown hash; a misaligned tree, in or paths; tree or root overlapping
 * in; root inside tree; paths overlapping tree, rows overlapping in; an index >= n.
 *
 * Declared in every product library over the library's own field element, libsppark_m31 and libsppark_bb31x4 included.
 */
#ifndef SPPARK_AMD_MERKLE_H
#define SPPARK_AMD_MERKLE_H

#include "sppark_amd.h"

#define SPPARK_HASH_BLAKE2S 0
#define SPPARK_HASH_SHA256  1
#define SPPARK_MERKLE_MAX_LG 28
#define SPPARK_MERKLE_DIGEST_BYTES 32
/* digests in a tree of 2^lg_n leaves: 2^(lg_n+1) - 1; layer l (0 = leaves .. lg_n = root) holds 2^(lg_n-l) digests
   and starts at digest index 2^(lg_n+1) - 2^(lg_n-l+1): layers lie bottom-up, the root is the last 32 bytes */
#define SPPARK_MERKLE_TREE_BYTES(lg_n) ((((size_t)2 << (lg_n)) - 1) * 32)

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_merkle_commit(size_t device_id, void *tree, void *root, const void *in, uint32_t lg_n, size_t width, size_t col_stride,
                              size_t leaf_stride, int hash, void *stream);
SppError sppark_merkle_open(size_t device_id, void *paths, const void *tree, uint32_t lg_n, const uint64_t *indices, size_t nidx,
                            void *stream);
SppError sppark_merkle_gather(size_t device_id, void *rows, const void *in, uint32_t lg_n, size_t width, size_t col_stride,
                              size_t leaf_stride, const uint64_t *indices, size_t nidx, void *stream);

#ifdef __cplusplus
}
#endif
#endif
