// MI355X kernels of the circle transform over Mersenne31 (include/sppark_amd_circle.h has the contract).
//
// The network.  Coefficients in natural order, evaluations in BITREV order.  Forward: layers b = k-1 ... 1 (x-layers)
// pair positions p and p + 2^b with the butterfly (u, v) -> (u + t v, u - t v), t = T_b(h) for the block h = p >> (b+1),
//        T_b(h) = x(g_{k+1}^((4 rev_{k-1-b}(h) + 1) 2^(b-1))),
// then the y-layer pairs 2h and 2h + 1 with t = y(g_{k+1}^(4 rev_{k-1}(h) + 1)).  Inverse: the layers in the opposite order
// with (u, v) -> (u + v, (u - v) / t) and one factor 1/n.
//
// A PASS runs S consecutive layers b_lo ... b_lo + S - 1 on a tile held in LDS: [2^S rows] x [2^lgC adjacent columns]
// of one column of the batch (rows = the bits b_lo ... of the position, columns = its lowest bits, so that every
// row of the tile is one contiguous segment of >= 64 bytes).  The pass on the lowest layers (b_lo = 0) takes 2^S
// contiguous elements; when the whole column is shorter than the tile, 2^(lgT - k) columns of the batch share a
// work-group and its twiddles (columns of 2^1 ... 2^6 elements: several to a wave).  Inside a pass the layers run in
// registers, four at a time (circle_round below).
//
// Twiddles of a tile.  A twiddle depends on the block only, not on the position inside it, so a tile needs one twiddle
// per block and layer: 2^S - 1 in all, kept in LDS next to the data (layer lb at tw[2^(S-1-lb) ... 2^(S-lb))).
//   forward   T_{b+1}(h) = pi(T_b(2h)), pi(x) = 2x^2 - 1: only the pass's LOWEST layer is computed from the group --
//             G^e out of three tables of 2^10 + 2^11 + 2^10 points (e < 2^31 split 10 | 11 | 10 bits, two group products,
//             32 KB per device whatever the size) -- and every layer above it costs one product per twiddle.  The
//             y-layer shares its points with layer 1: y(P) and -y(P) for the blocks 2h and 2h + 1.  That is 8 products
//             per point and about 2.3 per element of a low tile (against S/2 = 6 butterfly products per element); a high
//             tile needs 2^S twiddles for 2^12 elements.
//   inverse   1/t is not a coordinate of a point: the tiles read it from per-layer tables, L_m[h] = 1 / T_1(h) of
//             size m and Y_k[h] = 1 / y(...) of the even blocks (circle_driver.hpp builds and caches them).  Layer b of
//             size k uses L_{k-b+1}, so the tables of one size serve every larger one.
//
// Each round is a SPPARK_DEVFN function of (tid, nthreads) so that the host emulation (tests/emu/emu_circle.cpp)
// runs the same index math on the CPU.
#pragma once
#include "../ntt/ntt_kernels.hpp"       // bit_rev32, the k_bitrev* templates (NATURAL order)

namespace sppark_amd {

// Mersenne31 in canonical residues, mrs31_dev's memory image (ff/small_fields_dev.hpp), with reductions by ONE
// unsigned minimum -- min(s, s - p) is s - p exactly when that does not wrap -- where mrs31_dev compares and selects:
// a sum or a difference is 3 instructions, a product 6 (one 32 x 32 -> 64 multiply), a butterfly 12 instead of 17.
// The passes sit at the vector-instruction ceiling, so that is a quarter of their time.  Same values, bit for bit.
struct cm31_dev {
    static constexpr u32 MOD = 0x7fffffffu;
    typedef u32 word_t;
    u32 v;                                                      // [0, p)
    SPPARK_DEVFN static cm31_dev from_raw(u32 x) { cm31_dev r; r.v = x; return r; }
    SPPARK_DEVFN static cm31_dev one() { return from_raw(1); }
    SPPARK_DEVFN static u32 umin(u32 x, u32 y) { return x < y ? x : y; }
    SPPARK_DEVFN cm31_dev inverse() const { return field_pow(*this, (u64)MOD - 2); }   // a^(p-2); a != 0
    SPPARK_DEVFN friend cm31_dev operator+(cm31_dev a, cm31_dev b)
    {   const u32 s = a.v + b.v; return from_raw(umin(s, s - MOD));   }               // s < 2p: s - p wraps iff s < p
    SPPARK_DEVFN friend cm31_dev operator-(cm31_dev a, cm31_dev b)
    {   const u32 d = a.v - b.v; return from_raw(umin(d, d + MOD));   }               // d wrapped iff a < b; then d + p is the residue
    SPPARK_DEVFN friend cm31_dev operator*(cm31_dev a, cm31_dev b)
    {
        const u64 t = (u64)a.v * b.v;                           // <= (p-1)^2 < 2^62
        // 2^31 = 1: t = lo + 2^31 hi = lo + hi with lo <= p and hi <= (p-1)^2 >> 31 < p - 1, so the sum is below 2p and
        // one minimum reduces it
        const u32 r = (u32)(t & MOD) + (u32)(t >> 31);
        return from_raw(umin(r, r - MOD));
    }
};
typedef cm31_dev cf_t;
struct circle_pt { cf_t x, y; };

static constexpr u32 CIRCLE_GEN_X = 2, CIRCLE_GEN_Y = 1268011823;      // G, of order 2^31
static constexpr unsigned CIRCLE_MAX_LG = 30;
static constexpr unsigned CIRCLE_PT_LO = 10, CIRCLE_PT_MID = 11, CIRCLE_PT_HI = 10;    // the split of an exponent
static constexpr unsigned CIRCLE_PT_ENTRIES = (1u << CIRCLE_PT_LO) + (1u << CIRCLE_PT_MID) + (1u << CIRCLE_PT_HI);
static constexpr unsigned CIRCLE_MAX_S = 12;                           // layers of one pass (tile of 2^12 elements)

SPPARK_DEVFN circle_pt circle_mul(circle_pt a, circle_pt b)
{   circle_pt r; r.x = a.x * b.x - a.y * b.y; r.y = a.x * b.y + a.y * b.x; return r;   }
SPPARK_DEVFN cf_t circle_mul_x(circle_pt a, circle_pt b) { return a.x * b.x - a.y * b.y; }
SPPARK_DEVFN cf_t circle_pi(cf_t x) { const cf_t s = x * x; return s + s - cf_t::one(); }

// pts[i] = G^i (i < 2^10) | G^(i << 10) (i < 2^11) | G^(i << 21) (i < 2^10)
SPPARK_DEVFN circle_pt circle_gpow(const circle_pt* pts, u32 e)
{
    const circle_pt hi = pts[(1u << CIRCLE_PT_LO) + (1u << CIRCLE_PT_MID) + (e >> (CIRCLE_PT_LO + CIRCLE_PT_MID))];
    const circle_pt mid = pts[(1u << CIRCLE_PT_LO) + ((e >> CIRCLE_PT_LO) & ((1u << CIRCLE_PT_MID) - 1))];
    return circle_mul(circle_mul(hi, mid), pts[e & ((1u << CIRCLE_PT_LO) - 1)]);
}
SPPARK_DEVFN cf_t circle_gpow_x(const circle_pt* pts, u32 e)
{
    const circle_pt hi = pts[(1u << CIRCLE_PT_LO) + (1u << CIRCLE_PT_MID) + (e >> (CIRCLE_PT_LO + CIRCLE_PT_MID))];
    const circle_pt mid = pts[(1u << CIRCLE_PT_LO) + ((e >> CIRCLE_PT_LO) & ((1u << CIRCLE_PT_MID) - 1))];
    return circle_mul_x(circle_mul(hi, mid), pts[e & ((1u << CIRCLE_PT_LO) - 1)]);
}

// entry i of the point tables, by square and multiply from G (4096 entries, once per device)
SPPARK_DEVFN void circle_point_item(circle_pt* pts, unsigned i)
{
    u32 e = i;
    if (i >= (1u << CIRCLE_PT_LO) + (1u << CIRCLE_PT_MID)) e = (i - (1u << CIRCLE_PT_LO) - (1u << CIRCLE_PT_MID)) << (CIRCLE_PT_LO + CIRCLE_PT_MID);
    else if (i >= (1u << CIRCLE_PT_LO)) e = (i - (1u << CIRCLE_PT_LO)) << CIRCLE_PT_LO;
    circle_pt r, b;
    r.x = cf_t::one(); r.y = cf_t::from_raw(0);
    b.x = cf_t::from_raw(CIRCLE_GEN_X); b.y = cf_t::from_raw(CIRCLE_GEN_Y);
    for (; e; e >>= 1) { if (e & 1) r = circle_mul(r, b); b = circle_mul(b, b); }
    pts[i] = r;
}

// exponent of G whose x-coordinate is T_b(h) in a transform of 2^k elements (b >= 1); its y-coordinate, for b = 1, is the
// y-layer's twiddle of the block 2h
SPPARK_DEVFN u32 circle_tw_exp(unsigned k, unsigned b, u32 h)
{   return ((4u * bit_rev32(h, k - 1 - b) + 1u) << (b - 1)) << (CIRCLE_MAX_LG - k);   }

// entry h of L_m (want_y = 0) or Y_m (want_y = 1), h < 2^(m-2), m >= 2: one field inversion each, once per (device, m)
SPPARK_DEVFN void circle_inv_table_item(cf_t* out, const circle_pt* pts, unsigned m, int want_y, size_t h)
{
    const circle_pt q = circle_gpow(pts, circle_tw_exp(m, 1, (u32)h));
    out[h] = (want_y ? q.y : q.x).inverse();           // (never zero: q has order 2^(m+1) >= 8)
}

struct circle_pass {
    unsigned k;         // log2 of the column
    unsigned b_lo, S;   // the layers b_lo ... b_lo + S - 1
    unsigned lgC;       // log2 adjacent columns of the tile (0 when b_lo == 0)
    unsigned lgT;       // log2 elements of the tile: S + lgC, or more when columns of the batch are packed (k < lgT)
    unsigned vec;       // 16-byte global accesses (every column 16-byte aligned, k >= 2)
    unsigned pad_lg;    // elements at and above 2^pad_lg are READ as zero (the LDE's padding; >= k: none)
    u32 scale;          // the store multiplies by this (1/n, inverse) unless 0
    const cf_t* itw[CIRCLE_MAX_S];      // inverse: the table of layer b_lo + lb (null for the y-layer of k = 1)
};

// where element e of the tile lives: column |col| of the batch, position |p| in it
SPPARK_DEVFN bool circle_addr(const circle_pass& P, size_t tile, size_t y, size_t cols, unsigned e, size_t& col, size_t& p)
{
    if (P.k < P.lgT) {                                  // packed columns
        col = (y << (P.lgT - P.k)) + (e >> P.k); p = e & ((1u << P.k) - 1);
        return col < cols;
    }
    col = y;
    if (P.b_lo == 0) { p = (tile << P.lgT) + e; return true; }
    const unsigned row = e >> P.lgC, c = e & ((1u << P.lgC) - 1), cb = P.b_lo - P.lgC;
    const size_t chunk = tile & (((size_t)1 << cb) - 1), hi = tile >> cb;
    p = (hi << (P.b_lo + P.S)) | ((size_t)row << P.b_lo) | (chunk << P.lgC) | c;
    return true;
}
// the tile's part of the block index above its own rows
SPPARK_DEVFN u32 circle_tile_hi(const circle_pass& P, size_t tile)
{   return P.k < P.lgT ? 0u : (u32)(P.b_lo == 0 ? tile : tile >> (P.b_lo - P.lgC));   }

// LDS image of a tile: one pad word after every 16 elements, so that the lanes of the round on the lowest layers --
// each owning 16 ADJACENT elements -- spread over the banks
SPPARK_DEVFN unsigned circle_lds_index(unsigned e) { return e + (e >> 4); }
SPPARK_DEVFN unsigned circle_lds_elems(unsigned lgT) { return (1u << lgT) + ((1u << lgT) >> 4); }

struct alignas(16) circle_vec { cf_t e[4]; };

SPPARK_DEVFN void circle_load(const cf_t* data, size_t stride, size_t cols, cf_t* lds, const circle_pass& P, size_t tile, size_t y,
                              unsigned tid, unsigned nt)
{
    const size_t lim = (size_t)1 << (P.pad_lg < P.k ? P.pad_lg : P.k);
    if (P.vec) {
        // four 16-byte loads per lane in flight (a tile of 2^12 elements and 256 lanes: all of them) before the first LDS write
        for (unsigned e0 = 4 * tid; e0 < (1u << P.lgT); e0 += 16 * nt) {
            circle_vec v[4];
            #pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const unsigned e = e0 + 4 * nt * k;
                size_t col, p;
                v[k].e[0] = v[k].e[1] = v[k].e[2] = v[k].e[3] = cf_t::from_raw(0);
                if (e < (1u << P.lgT) && circle_addr(P, tile, y, cols, e, col, p) && p < lim)
                    v[k] = *reinterpret_cast<const circle_vec*>(data + col * stride + p);
            }
            #pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const unsigned e = e0 + 4 * nt * k;
                if (e < (1u << P.lgT)) for (unsigned j = 0; j < 4; j++) lds[circle_lds_index(e + j)] = v[k].e[j];
            }
        }
        return;
    }
    for (unsigned e = 4 * tid; e < (1u << P.lgT); e += 4 * nt) {
        size_t col, p;
        {
            for (unsigned j = 0; j < 4 && e + j < (1u << P.lgT); j++)
                lds[circle_lds_index(e + j)] = circle_addr(P, tile, y, cols, e + j, col, p) && p < lim ? data[col * stride + p] : cf_t::from_raw(0);
        }
    }
}

SPPARK_DEVFN void circle_store(cf_t* data, size_t stride, size_t cols, const cf_t* lds, const circle_pass& P, size_t tile, size_t y,
                               unsigned tid, unsigned nt)
{
    const cf_t sc = cf_t::from_raw(P.scale);
    for (unsigned e = 4 * tid; e < (1u << P.lgT); e += 4 * nt) {
        size_t col, p;
        if (P.vec) {
            if (!circle_addr(P, tile, y, cols, e, col, p)) continue;
            circle_vec v;
            for (unsigned j = 0; j < 4; j++) v.e[j] = P.scale ? lds[circle_lds_index(e + j)] * sc : lds[circle_lds_index(e + j)];
            *reinterpret_cast<circle_vec*>(data + col * stride + p) = v;
        } else {
            for (unsigned j = 0; j < 4 && e + j < (1u << P.lgT); j++)
                if (circle_addr(P, tile, y, cols, e + j, col, p))
                    data[col * stride + p] = P.scale ? lds[circle_lds_index(e + j)] * sc : lds[circle_lds_index(e + j)];
        }
    }
}

// the tile's twiddles into tw[2^S]: layer lb (b = b_lo + lb), block j of the tile at tw[2^(S-1-lb) + j]
template<bool INV>
SPPARK_DEVFN void circle_twiddles(cf_t* tw, const circle_pass& P, const circle_pt* pts, size_t tile, unsigned tid, unsigned nt)
{
    const u32 hi = circle_tile_hi(P, tile);
    const unsigned S = P.S;
    if (INV) {
        for (unsigned lb = 0; lb < S; lb++) {
            const unsigned b = P.b_lo + lb, cnt = 1u << (S - 1 - lb);
            const cf_t* tab = P.itw[lb];
            for (unsigned j = tid; j < cnt; j += nt) {
                const size_t h = ((size_t)hi << (S - 1 - lb)) | j;
                cf_t t;
                if (b) t = tab[h];
                else if (P.k == 1) t = cf_t::from_raw(cf_t::MOD - 1);          // 1 / y(g_2) = -1
                else { t = tab[h >> 1]; if (h & 1) t = cf_t::from_raw(0) - t; }
                tw[cnt + j] = t;
            }
        }
        return;
    }
    if (P.b_lo == 0 && S == 1) {                                               // k = 1: the y-layer alone, t = y(g_2)
        if (tid == 0) tw[1] = circle_gpow(pts, 1u << (CIRCLE_MAX_LG - 1)).y;
        return;
    }
    if (P.b_lo == 0) {                                                         // points of layer 1; the y-layer shares them
        const unsigned cnt = 1u << (S - 2);
        for (unsigned j = tid; j < cnt; j += nt) {
            const circle_pt q = circle_gpow(pts, circle_tw_exp(P.k, 1, (hi << (S - 2)) | j));
            tw[(1u << (S - 1)) + 2 * j] = q.y;
            tw[(1u << (S - 1)) + 2 * j + 1] = cf_t::from_raw(0) - q.y;
            tw[cnt + j] = q.x;
            cf_t x = q.x;
            for (unsigned lb = 2; lb < S && (j & ((1u << (lb - 1)) - 1)) == 0; lb++) {
                x = circle_pi(x);
                tw[(1u << (S - 1 - lb)) + (j >> (lb - 1))] = x;
            }
        }
        return;
    }
    const unsigned cnt = 1u << (S - 1);
    for (unsigned j = tid; j < cnt; j += nt) {
        cf_t x = circle_gpow_x(pts, circle_tw_exp(P.k, P.b_lo, (hi << (S - 1)) | j));
        tw[cnt + j] = x;
        for (unsigned lb = 1; lb < S && (j & ((1u << lb) - 1)) == 0; lb++) {
            x = circle_pi(x);
            tw[(1u << (S - 1 - lb)) + (j >> lb)] = x;
        }
    }
}

// The S layers of a pass run in ceil(S / 4) ROUNDS of R <= 4 layers, nearly equal: a lane takes the 2^R elements
// that R consecutive layers combine into registers, runs the R layers there and puts them back -- one LDS read and
// one LDS write per element and ROUND (not per layer), 2^R - 1 twiddle reads per 2^R elements, a barrier per round.
SPPARK_DEVFN unsigned circle_rounds(unsigned S) { return (S + 3) / 4; }
SPPARK_DEVFN void circle_round_span(unsigned S, unsigned i, unsigned& lb0, unsigned& R)
{
    const unsigned nr = circle_rounds(S), base = S / nr, extra = S % nr;
    R = base + (i < extra ? 1 : 0);
    lb0 = i * base + (i < extra ? i : extra);
}

// the layers lb0 ... lb0 + R - 1 of the pass: rows r and r + 2^lb are LDS positions 2^(lb + lgC) apart
template<bool INV, unsigned R>
SPPARK_DEVFN void circle_round(cf_t* lds, const cf_t* tw, const circle_pass& P, unsigned lb0, unsigned tid, unsigned nt)
{
    const unsigned L0 = lb0 + P.lgC;
    for (unsigned g = tid; g < (1u << (P.lgT - R)); g += nt) {
        const unsigned low = g & ((1u << L0) - 1), high = g >> L0, base = (high << (L0 + R)) | low;
        cf_t x[1u << R];
        #pragma unroll
        for (unsigned i = 0; i < (1u << R); i++) x[i] = lds[circle_lds_index(base + (i << L0))];
        #pragma unroll
        for (unsigned s = 0; s < R; s++) {
            const unsigned r = INV ? s : R - 1 - s;                             // the layer lb0 + r
            const unsigned cnt = 1u << (P.S - 1 - lb0 - r);                     // its blocks in the tile (per packed column)
            cf_t t[1u << (R - 1)];                                              // (2^(R-1-r) of them are used)
            #pragma unroll
            for (unsigned c = 0; c < (1u << (R - 1 - r)); c++) t[c] = tw[cnt + (((high << (R - 1 - r)) | c) & (cnt - 1))];
            #pragma unroll
            for (unsigned q = 0; q < (1u << (R - 1)); q++) {
                const unsigned i = ((q >> r) << (r + 1)) | (q & ((1u << r) - 1)), j = i + (1u << r);
                const cf_t u = x[i], v = x[j];
                if (INV) { x[i] = u + v; x[j] = (u - v) * t[i >> (r + 1)]; }
                else     { const cf_t w = v * t[i >> (r + 1)]; x[i] = u + w; x[j] = u - w; }
            }
        }
        #pragma unroll
        for (unsigned i = 0; i < (1u << R); i++) lds[circle_lds_index(base + (i << L0))] = x[i];
    }
}
// round |i| of the pass (rounds are numbered from the lowest layers)
template<bool INV>
SPPARK_DEVFN void circle_round_at(cf_t* lds, const cf_t* tw, const circle_pass& P, unsigned i, unsigned tid, unsigned nt)
{
    unsigned lb0, R;
    circle_round_span(P.S, i, lb0, R);
    if (R == 4) circle_round<INV, 4>(lds, tw, P, lb0, tid, nt);
    else if (R == 3) circle_round<INV, 3>(lds, tw, P, lb0, tid, nt);
    else if (R == 2) circle_round<INV, 2>(lds, tw, P, lb0, tid, nt);
    else circle_round<INV, 1>(lds, tw, P, lb0, tid, nt);
}

#if defined(__HIPCC__)
// grid: x = tiles of a column (1 when columns are packed), y = columns (or groups of packed columns); dynamic LDS:
// (circle_lds_elems(lgT) + 2^S) elements
template<bool INV>
__global__ __launch_bounds__(256)
void k_circle_pass(cf_t* data, size_t stride, size_t cols, circle_pass P, const circle_pt* pts)
{
    extern __shared__ unsigned char circle_lds[];
    cf_t* lds = reinterpret_cast<cf_t*>(circle_lds);
    cf_t* tw = lds + circle_lds_elems(P.lgT);
    const size_t tile = blockIdx.x, y = blockIdx.y;
    circle_load(data, stride, cols, lds, P, tile, y, threadIdx.x, blockDim.x);
    circle_twiddles<INV>(tw, P, pts, tile, threadIdx.x, blockDim.x);
    __syncthreads();
    const unsigned nr = circle_rounds(P.S);
    for (unsigned i = 0; i < nr; i++) {
        circle_round_at<INV>(lds, tw, P, INV ? i : nr - 1 - i, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    circle_store(data, stride, cols, lds, P, tile, y, threadIdx.x, blockDim.x);
}

// (templates so that only the translation unit that launches them holds a copy)
template<class PT>
__global__ __launch_bounds__(256) void k_circle_points(PT* pts)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < CIRCLE_PT_ENTRIES) circle_point_item(pts, i);
}

template<class PT>
__global__ __launch_bounds__(256) void k_circle_inv_table(cf_t* out, const PT* pts, unsigned m, int want_y)
{
    const size_t h = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h < ((size_t)1 << (m - 2))) circle_inv_table_item(out, pts, m, want_y, h);
}
#endif

} // namespace sppark_amd
