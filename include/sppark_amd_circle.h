/*
 * sppark_amd circle transform over Mersenne31 (p = 2^31 - 1): evaluate, interpolate and low-degree extension of
 * polynomials over the circle group.  p - 1 has 2-adicity 1, so the field has no radix-2 NTT; the circle group
 * x^2 + y^2 = 1 has order 2^31 and carries the transform used with this field.  The reference has no counterpart.
 * Exported by libsppark_m31 only.  Elements are canonical residues in [0, p), four bytes each, as everywhere in that
 * library; outputs are canonical.
 *
 * THE CONTRACT (this definition, nothing else, is what the entry points compute)
 *   group       C = {(x, y) in F_p^2 : x^2 + y^2 = 1},  (x0, y0)(x1, y1) = (x0 x1 - y0 y1, x0 y1 + y0 x1)
 *   generator   G = (2, 1268011823) has order 2^31;  g_m = G^(2^(31-m)) has order 2^m
 *   squaring    pi(x) = 2x^2 - 1 is the x-coordinate of P^2 when x is the x-coordinate of P
 *   domain D_k of n = 2^k points, 1 <= k <= 30:  H_i = g_{k+1}^(4i+1) for 0 <= i < n/2;  D_i = H_i for i < n/2,
 *               D_i = conj(H_{i-n/2}) = (x, -y) for i >= n/2.  D_k and D_{k+b} are disjoint for b >= 1.
 *   basis       for a coefficient index j with bits j_0 (lowest) ... j_{k-1}:
 *               b_j(x, y) = y^j_0 x^j_1 pi(x)^j_2 pi^2(x)^j_3 ... pi^(k-2)(x)^j_{k-1}
 *               (b_j does not depend on k: zero-padding a coefficient vector leaves the polynomial unchanged)
 *   forward     e_i = sum_j c_j b_j(D_i); coefficients always in natural index order
 *   inverse     the inverse map, the factor 1/n included
 *   evaluation order   SPPARK_CIRCLE_EVALS_BITREV: position q holds e_{bitrev_k(q)} (what the in-place network gives for
 *               free);  SPPARK_CIRCLE_EVALS_NATURAL: position i holds e_i (one more pass over the data)
 *   k = 0       one element; every call is the identity
 * Anchors (p - 1 = 2147483646):  g_2 = (0, 2147483646);  g_3 = (32768, 2147450879);
 *   D_1 = [(0, 2147483646), (0, 1)];  D_2 = [(32768, 2147450879), (2147450879, 32768), (32768, 32768), (2147450879, 2147450879)];
 *   coefficients [1, 2, 3, 4] at k = 2 give natural-order evaluations [32767, 2147450878, 163843, 2147319810];
 *   [1 .. 8] at k = 3 give [885347334, 714723476, 1262332919, 1432563561, 2092305986, 1109642644, 55636419, 1037382257].
 * This is believed to be the canonic-coset circle domain with bit-reversed evaluations that circle-STARK provers use, but
 * it has NOT been checked against any of them: no compatibility with another implementation is claimed.  A caller who
 * needs one should compare the anchors above (and sppark_amd.circle.domain) first.
 *
 * sppark_circle_ntt: |batch| in-place transforms of 2^lg elements.  Column j is inout[j*stride .. j*stride + 2^lg);
 *   |stride| is in elements, 0 means 2^lg, otherwise at least 2^lg.  Elements between columns are never read or written.
 *   FORWARD: coefficients -> evaluations on D_lg in |evals_order|; INVERSE: evaluations in |evals_order| -> coefficients.
 *   Every column gets, bit for bit, what a call with batch = 1 gives it.  Columns that start 16-byte aligned move
 *   16 bytes per access.
 * sppark_circle_lde: |batch| low-degree extensions.  Column j owns inout[j*ext .. (j+1)*ext), ext = 2^(lg+lg_blowup); its
 *   first 2^lg elements hold the evaluations on D_lg in |evals_order|, the rest is never read.  On return the column
 *   holds the evaluations of the same polynomial on D_(lg+lg_blowup) in the same order.  aux_out is NULL or receives
 *   batch x 2^lg packed elements: column j's coefficients at aux_out + j*2^lg.  (Interpolate, copy, then evaluate the
 *   zero-padded coefficients; the padding rides in the first forward pass's load.)
 * sppark_circle_cached_bytes / sppark_circle_release_cached: the device memory the library keeps for |device_id| between
 *   calls -- 32 KB of group elements for the forward twiddles, and the inverse twiddles of every size used so far up to
 *   2^24 -- never more than SPPARK_CIRCLE_CACHE_CAP_BYTES; release frees all of it (it waits for the device first), the
 *   next call rebuilds what it needs.  Do not call release while another thread runs a circle call on that device: the
 *   wait covers enqueued work only, not a call that has fetched its tables and not launched yet.
 *
 * No-ops: batch == 0, and lg == 0 for sppark_circle_ntt.  Pointers may be host or device pointers; host columns are
 * staged through the library's scratch pool, packed.  Streams: sppark_circle_ntt on a device buffer with a non-NULL
 * stream only enqueues its launches -- except that a call which has to BUILD tables (the first forward call on a device,
 * the first inverse call of a size) synchronises the stream once, before the tables enter the cache, and an inverse above 2^24 (tables in call scratch)
 * synchronises before it returns.  Everything else returns when the result is in place.
 * Rejected before a device is looked up (negated hipErrorInvalidValue, owned message): lg (+ lg_blowup) above
 * SPPARK_CIRCLE_MAX_LG, an order or direction outside its enum, 0 < stride < 2^lg, extents that overflow size_t, a NULL
 * buffer with work to do.
 *
 * How it runs (DESIGN.md "Circle transform over M31"): the lowest 12 layers are one launch on contiguous 16 KB tiles in
 * LDS, the layers above them launches of at most 8 layers on tiles of [2^S rows] x [2^(12-S) columns]: 1 launch up to
 * 2^12, 2 up to 2^20, 3 up to 2^28.  Columns are grid rows; columns shorter than a tile share a work-group (columns of
 * up to 2^6 elements: several to a wave); a batch above the grid limit is split into launches.  Forward twiddles are never
 * read from a table of the transform's size: each tile computes its lowest layer's from G^e (4096 points per device, two
 * group products) and steps to the next layer with pi(x), one product.  Inverse twiddles are field inverses -- 1/x of a
 * point's coordinate is no coordinate of a point -- and are read from cached tables: at most one column's size of device
 * memory beyond inout, whatever the batch.
 *
 * Measured on one MI355X (profiles/r11_circle_ntt.log; device buffers, non-NULL stream): one forward transform takes 0.019 /
 * 0.025 / 0.174 ms at 2^16 / 2^20 / 2^24 (NATURAL order 0.022 / 0.030 / 0.201), against 0.008 / 0.017 / 0.090 ms for libsppark_bb31's
 * NTT of the same size: 1.49 / 1.20 / 1.46 times the target "that NTT plus one sppark_field_add over the array", which is
 * MISSED -- the 12-layer pass is bound by vector-instruction issue and LDS, at three times its memory floor.  The inverse
 * takes 0.98 - 0.99 of the forward time with warm tables and 0.114 / 0.138 / 0.444 ms on the first call of a size (tables
 * built).  4096 columns of 2^12: 0.094 ms forward, 0.079 inverse, against 0.174 / 0.172 for one transform of 2^24 (target:
 * no slower -- met).  64 LDEs 2^16 -> 2^18: 0.169 ms.  DESIGN.md "Circle transform over M31" has the table and the account.
 */
#ifndef SPPARK_AMD_CIRCLE_H
#define SPPARK_AMD_CIRCLE_H

#include "sppark_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPPARK_CIRCLE_MAX_LG 30
/* the inverse twiddles of the sizes 2^2 .. 2^24 (two families of 2^(m-2) elements) and 4096 group elements */
#define SPPARK_CIRCLE_CACHE_CAP_BYTES (((size_t)64 << 20) + ((size_t)32 << 10))
enum { SPPARK_CIRCLE_EVALS_BITREV = 0, SPPARK_CIRCLE_EVALS_NATURAL = 1 };
enum { SPPARK_CIRCLE_FORWARD = 0, SPPARK_CIRCLE_INVERSE = 1 };

SppError sppark_circle_ntt(size_t device_id, void *inout, uint32_t lg, size_t batch, size_t stride,
                           int evals_order, int direction, void *stream);
SppError sppark_circle_lde(size_t device_id, void *inout, uint32_t lg, uint32_t lg_blowup, size_t batch,
                           int evals_order, void *aux_out, void *stream);
size_t   sppark_circle_cached_bytes(size_t device_id);
SppError sppark_circle_release_cached(size_t device_id);

#ifdef __cplusplus
}
#endif
#endif
