/*
 * sppark_amd Poseidon2: the permutation over BabyBear and Goldilocks and Merkle commitments hashed with it, for provers
 * whose verifier is itself proved (recursion wants a hash that is cheap as a circuit).  The tree is the tree of
 * sppark_amd_merkle.h, a digest is 32 bytes there and here: sppark_merkle_open, sppark_merkle_gather and the layer
 * arithmetic serve a Poseidon2 tree unchanged.  The reference's snapshot has no hash of any kind.
 *
 * 1. The permutation.  Field F is the library's field.  Width T = 16 for BabyBear (libsppark_bb31, libsppark_bb31_canonical),
 * T = 8 for Goldilocks (libsppark_gl64, libsppark_gl64_plonky2).  S-box x -> x^7 in both fields: 7 is the smallest exponent
 * coprime to p - 1 in both (p - 1 = 15 * 2^27 and p - 1 = 2^32 * 3 * 5 * 17 * 257 * 65537).
 *   External layer M_E.  M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]].  Split x into T/4 blocks of 4 and compute
 *     z_b = M4 x_b for each block; s = sum_b z_b, a 4-vector; output y_b = z_b + s.  This is circ(2 M4, M4, ..).
 *   Internal layer M_I.  s = sum_i x_i; y_i = d_i x_i + s.  The diagonal d_0 .. d_{T-1} is data.
 *   Permutation.  First x <- M_E x.  Then RF/2 full rounds: a full round adds ce[r][i] to every x_i, applies the S-box to
 *     every x_i, then applies M_E.  Then RP partial rounds: a partial round adds ci[r] to x_0, applies the S-box to x_0
 *     only, then applies M_I.  Then the remaining RF/2 full rounds.
 * The parameters are the caller's: rounds_f (even, 2 .. 16), rounds_p (0 .. 64) and ONE constants buffer of
 * rounds_f * T + rounds_p + T field elements in the library's wire format (sppark_amd.h, section 3: Montgomery words with
 * R = 2^32 for BabyBear, canonical integers for Goldilocks): the external constants round by round (ce[r][i] at r * T + i),
 * then the internal constants, then the diagonal.  The buffer may lie on the host or on the device.  The diagonal is
 * multiplied generically, so any parameter set works; no constant set is built into the library.
 *
 * This is the structure of the Poseidon2 paper (Grassi, Khovratovich, Schofnegger, 2023) as Plonky3 instantiates it; the
 * usual parameters are RF = 8 with RP = 13 for BabyBear-16 and RF = 8 with RP = 22 for Goldilocks-8.  Compatibility with any
 * other implementation is believed, NOT compared: no outside implementation or test vector was at hand when this was
 * written.  A caller who needs it loads their prover's constants into the buffer and compares a permutation first.
 *
 * 2. Hashing.  RATE = OUT = T/2: 8 for BabyBear, 4 for Goldilocks.  A digest is OUT elements in wire format, 32 bytes.
 *   Leaf.  A padding-free overwrite sponge over the width elements of the leaf, in column order j = 0 .. width - 1.  The state
 *     starts at zero.  For every chunk of RATE elements the chunk's elements overwrite state[0 .. len - 1], then the state is
 *     permuted.  A last partial chunk overwrites only its own positions and is followed by one permutation.  There is no
 *     padding and no length word: leaves of different widths are not domain-separated, a tree has one width.
 *     The digest is state[0 .. OUT - 1].
 *   Node.  state = left || right, one permutation, digest = state[0 .. OUT - 1]: a truncated permutation, no feed-forward.
 *   Tree.  Exactly the layout of sppark_amd_merkle.h: layers bottom-up, the root in the last 32 bytes; lg_n = 0 makes the leaf
 *     digest the root.
 * Inputs are taken as stored.  Elements and constants are expected canonical (below p), as the library's own outputs are;
 * words that are not are NOT detected and what they hash to is unspecified.
 *
 * sppark_poseidon2_permute  count states of T elements (64 bytes each), out and in 16-byte aligned, host or device;
 *   out == in is allowed, any other overlap is not.  count == 0 does nothing.  One launch.
 * sppark_poseidon2_commit   the matrix arguments (in, lg_n, width, col_stride, leaf_stride), tree and root are those of
 *   sppark_merkle_commit, with its layouts, alignment and overlap rules and lg_n <= 28.  Two launches up to lg_n = 10,
 *   2 + ceil((lg_n - 10) / 3) above.
 * With every buffer on the device, consts included, and a stream that is not NULL the calls only enqueue their launches --
 * no allocation, no copy, no synchronisation.  Otherwise host buffers are staged through the device and the call returns
 * when the results are in place.
 *
 * Rejected before a device is looked up (negated hipErrorInvalidValue, owned message): everything sppark_merkle_commit
 * rejects, in its order; NULL or misaligned consts; consts overlapping tree, root or out; rounds_f odd or outside 2 .. 16;
 * rounds_p > 64; for permute NULL or misaligned out / in, count * 64 overflowing size_t, out and in overlapping in part.
 *
 * Exported by libsppark_bb31, libsppark_bb31_canonical, libsppark_gl64 and libsppark_gl64_plonky2 only.
 */
#ifndef SPPARK_AMD_POSEIDON2_H
#define SPPARK_AMD_POSEIDON2_H

#include "sppark_amd_merkle.h"

#define SPPARK_POSEIDON2_MAX_ROUNDS_F 16
#define SPPARK_POSEIDON2_MAX_ROUNDS_P 64
#define SPPARK_POSEIDON2_STATE_BYTES 64
/* elements of the constants buffer for a state of t elements (16: BabyBear, 8: Goldilocks) */
#define SPPARK_POSEIDON2_CONSTS(t, rounds_f, rounds_p) ((size_t)(rounds_f) * (t) + (rounds_p) + (t))

#ifdef __cplusplus
extern "C" {
#endif

SppError sppark_poseidon2_permute(size_t device_id, void *out, const void *in, size_t count,
                                  const void *consts, uint32_t rounds_f, uint32_t rounds_p, void *stream);
SppError sppark_poseidon2_commit(size_t device_id, void *tree, void *root, const void *in, uint32_t lg_n, size_t width,
                                 size_t col_stride, size_t leaf_stride,
                                 const void *consts, uint32_t rounds_f, uint32_t rounds_p, void *stream);

#ifdef __cplusplus
}
#endif
#endif
