// pq_ivf_kernels.hpp -- device code of the IVFPQ index (pq_index.hip): m codes and a label are ALL the index keeps of a row.  One index
// with two code widths, bits = 8 or 4 (bit_size): ksub = 1 << bits entries per sub-quantiser, cpw = 32 / bits codes per word.
//
//   codebooks : m sub-quantisers of ksub entries, cb[s][j] of dsub = dim / m floats; on the device in the order of pq_cb_index, which
//               makes the loads of the lanes that work on neighbouring entries contiguous;
//   decode    : x^[s * dsub + t] = fl(c_l[s * dsub + t] + cb[s][code[s]][t]);
//   sub-score : e(s, j) = sum over t ascending, sequential from +0, of fl(fl(q_t - x^_t)^2) (L2) or fl(q_t * x^_t) (IP, cosine);
//   encode    : code[s] = argmin_j of the L2 sub-score of the stored row against x^ (key = ordered word of e, then j; NaN never wins);
//   distance  : dis = +0, then dis = fl(dis + e(s, code[s])) for s = 0 .. m - 1: the ADC sum over a per-(query, list) table.
//
// Stored codes: a row is mw = ceil(m / cpw) 32-bit words (code s in bits bits * (s % cpw) .. of word s / cpw, zero padded); the rows,
// list-major, are kept in blocks of 64 TRANSPOSED: word w of row r is codes[((r / 64) * mw + w) * 64 + r % 64].  The scan takes one row
// per lane, so a wavefront's load of word w is 256 contiguous bytes (two pieces where its 64 rows straddle a block).  pq_code_word is
// the map.
//
// The scan is ONE kernel for both widths (pq_ivf_scan_kernel<BITS, ...>): the tables are 4 * ksub * m bytes per query, so at 4 bits
// tiles of up to 8 queries fit the LDS at every m <= 256.  The encoders are two algorithms (a block per row at 256 entries, 16 lanes
// per row at 16) over the same sub-score and lane-minimum helpers.
//
// query_tables=1 is a second definition of a row's distance over the same codebooks and codes, with tables that depend on the query
// alone (below, "the query-table form"): its two kernels, and the scan's FORM = 1.
#pragma once

#include "scan_kernels.hpp"

namespace msvs
{

// The whole LDS of a CU: the 8-bit look-up tables are T * m KiB.  pq_fits (pq_index.hip) admits shapes whose T = 1 image is EXACTLY this
// (dim 2816, m 128), so pq_ivf_scan_kernel and everything it calls (tile_rank_merge, WaveTopK) must keep every LDS byte inside the
// dynamic image that pq_lds_bytes counts: a static __shared__ variable anywhere on that path makes such an index fail at launch
// (pq_launch checks the compiled kernel's static LDS once and refuses to run rather than let that happen unnoticed).
constexpr size_t PQ_LDS_BUDGET = 160 * 1024;

/// index of word w of (list-major) row r in the stored codes, rows of mw words
__host__ __device__ inline size_t pq_code_word(size_t r, uint32_t w, uint32_t mw) { return ((r >> 6) * mw + w) * 64 + (r & 63); }

/// floats between the entries u and u + 1 of one codebook entry in the device copy of the codebooks.  8 bits: 256.  4 bits: 16 for
/// every sub-space of the group of four that s belongs to (the last group has m % 4 of them when 4 does not divide m)
template <int BITS>
__host__ __device__ inline uint32_t pq_cb_stride(uint32_t s, uint32_t m)
{
    return BITS == 8 ? 256u : (m - (s & ~3u) < 4u ? m - (s & ~3u) : 4u) * 16;
}

/// index of cb[s][j][u] in that copy, ksub * dim floats in all, no padding.  8 bits: [s][u][j], so thread j of a block reads entry j
/// and a wavefront's loads are contiguous.  4 bits: [group of four sub-spaces][u][sub-space in the group][j]: the 64 lanes of a
/// wavefront that build tables are (4 consecutive sub-spaces) x (16 entries), so their load at step u is 256 contiguous bytes; the 16
/// lanes that encode one row read 64 contiguous bytes.
/// The two 8-bit device sites (pq_encode_kernel, the scan's table build) spell `cbT + pq_cb_index<8>(s, 0, j, ...)` out as
/// `cbT + (size_t)s * dsub * 256 + j`: through the call the compiler folds the float scale into the index one pass later and all 24
/// 8-bit scans and the encoder come out with other registers and schedules.
template <int BITS>
__host__ __device__ inline size_t pq_cb_index(uint32_t s, uint32_t u, uint32_t j, uint32_t m, uint32_t dsub)
{
    return BITS == 8 ? ((size_t)s * dsub + u) * 256 + j : (size_t)(s >> 2) * dsub * 64 + (size_t)u * pq_cb_stride<4>(s, m) + (s & 3) * 16 + j;
}

// ------------------------------------------------------------------------------------------ training residuals

/// dst[i] = src[floor((i0 + i) * n / cap)] for i < cnt: the evenly spaced training rows (dense rows of d floats)
static __global__ void pq_pick_rows_kernel(const float * src, size_t n, size_t cap, size_t i0, size_t cnt, uint32_t d, float * dst)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cnt * d)
        return;
    const size_t i = e / d;
    const uint32_t j = (uint32_t)(e - i * d);
    const size_t r = (i0 + i) * n / cap; // (cap <= 2^18: no overflow below 2^46 rows)
    dst[e] = src[r * d + j];
}

/// R[i][j] = fl(X[i][j] - C[list[i]][j]): n rows of stride ld -> dense rows of d floats
static __global__ void pq_residual_kernel(const float * X, const int32_t * list, const float * C, size_t n, uint32_t d, uint32_t ld, float * R)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * d)
        return;
    const size_t i = e / d;
    const uint32_t j = (uint32_t)(e - i * d);
    R[e] = __fsub_rn(X[i * ld + j], C[(size_t)list[i] * ld + j]);
}

// ------------------------------------------------------------------------------------------ encode

/// the minimum over each group of W consecutive lanes, in all of them
template <int W>
__device__ __forceinline__ uint64_t pq_lane_min(uint64_t v)
{
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1)
    {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        v = other < v ? other : v;
    }
    return v;
}

/// the argmin key (ordered word of e, then j) of codebook entry j -- cb points at its first float, the next is gw floats on -- for
/// the columns c0 .. c0 + dsub - 1 of the row x against the centroid c; KEY_NONE where e is NaN (a NaN score never wins)
__device__ __forceinline__ uint64_t pq_encode_key(const float * x, const float * c, uint32_t c0, const float * cb, uint32_t gw, uint32_t dsub,
                                                  uint32_t j)
{
    float e = 0.f;
    for (uint32_t t = 0; t < dsub; t++)
    {
        const float xh = __fadd_rn(c[c0 + t], cb[(size_t)t * gw]);
        const float df = __fsub_rn(x[c0 + t], xh);
        e = __fadd_rn(e, __fmul_rn(df, df));
    }
    return e == e ? ((uint64_t)f2ord(e) << 32 | j) : KEY_NONE;
}

/// 8 bits: codes[r][s] (rows of mp = 4 * mw bytes, bytes m .. mp - 1 untouched) = code of sub-space s of row r against the centroid
/// of list[r].  A block takes rows_per_block rows, thread j codebook entry j; the row and its centroid are staged in LDS (dynamic: 2 * d floats);
/// the block argmin is over the key (ordered word of e, j).  One barrier per (row, sub-space): the wave minima alternate between two
/// LDS slots.
static __global__ __launch_bounds__(BLOCK) void pq_encode_kernel(const float * X, const int32_t * list, const float * C, const float * cbT,
                                                                 size_t n, uint32_t d, uint32_t ld, uint32_t m, uint32_t dsub, uint32_t mp,
                                                                 uint32_t rows_per_block, uint8_t * codes)
{
    float * xs = reinterpret_cast<float *>(msvs_smem); // [d] the stored row
    float * cs = xs + d;                               // [d] its list's centroid
    __shared__ uint64_t red[2][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r0 = (size_t)blockIdx.x * rows_per_block;
    const size_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    for (size_t r = r0; r < r1; r++)
    {
        __syncthreads(); // the previous row is done with xs / cs
        const float * x = X + r * ld;
        const float * c = C + (size_t)list[r] * ld;
        for (uint32_t i = tid; i < d; i += BLOCK)
        {
            xs[i] = x[i];
            cs[i] = c[i];
        }
        __syncthreads();
        for (uint32_t s = 0; s < m; s++)
        {
            const float * cb = cbT + (size_t)s * dsub * 256 + tid; // (pq_cb_index<8>(s, 0, tid, m, dsub), spelled out: see there)
            const uint64_t key = pq_lane_min<64>(pq_encode_key(xs, cs, s * dsub, cb, pq_cb_stride<8>(s, m), dsub, tid));
            if (lane == 0)
                red[s & 1][wave] = key;
            __syncthreads();
            if (tid == 0)
            {
                uint64_t best = red[s & 1][0];
#pragma unroll
                for (int w = 1; w < 4; w++)
                    best = red[s & 1][w] < best ? red[s & 1][w] : best;
                codes[r * mp + s] = best == KEY_NONE ? (uint8_t)0 : (uint8_t)(best & 255u);
            }
        }
    }
}

/// 4 bits: codes[r][s / 2] (rows of mp = 4 * mw bytes; bytes ceil(m / 2) .. mp - 1 untouched) holds code s in its low (s even) or
/// high nibble.  A block takes 16 rows, 16 lanes a row, lane j entry j; the argmin over the key (ordered word of e, j) is four shuffles.  Lane 0 of a row collects two codes and writes the whole byte: no byte has two writers.
/// Rows beyond n are computed as row n - 1 and not written (every lane stays in the shuffles); n >= 1.
static __global__ __launch_bounds__(BLOCK) void pq4_encode_kernel(const float * X, const int32_t * list, const float * C, const float * cb4,
                                                                  size_t n, uint32_t ld, uint32_t m, uint32_t dsub, uint32_t mp, uint8_t * codes)
{
    const uint32_t tid = threadIdx.x, j = tid & 15;
    const size_t r = (size_t)blockIdx.x * 16 + (tid >> 4);
    const size_t rc = r < n ? r : n - 1;
    const float * x = X + rc * ld;
    const float * c = C + (size_t)list[rc] * ld;
    uint32_t byte = 0;
    for (uint32_t s = 0; s < m; s++)
    {
        const uint64_t best = pq_lane_min<16>(pq_encode_key(x, c, s * dsub, cb4 + pq_cb_index<4>(s, 0, j, m, dsub), pq_cb_stride<4>(s, m), dsub, j));
        const uint32_t code = best == KEY_NONE ? 0u : (uint32_t)(best & 15u);
        byte = (s & 1) ? byte | code << 4 : code;
        if (j == 0 && r < n && ((s & 1) || s + 1 == m))
            codes[r * mp + (s >> 1)] = (uint8_t)byte;
    }
}

/// dst[pq_code_word(pos[r], w)] = src[r][w] for n staged rows of mw words (the staged chunks into their list-major places)
static __global__ void pq_scatter_rows_kernel(const uint32_t * src, uint32_t * dst, const uint32_t * pos, size_t n, uint32_t mw)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * mw)
        return;
    const size_t r = i / mw;
    dst[pq_code_word(pos[r], (uint32_t)(i - r * mw), mw)] = src[i];
}

// ------------------------------------------------------------------------------------------ the query-table form (query_tables=1)
//
//   query table : P[s][j] = sum over t ascending, sequential from +0, of fl(q[s * dsub + t] * cb[s][j][t]): no list in it;
//   row term    : (L2) g(s) = the same kind of sum of fl(cb_t * fl(fl(c_t + c_t) + cb_t)), cb = cb[s][code[s]], c_t = c_l[s * dsub + t];
//                 w = +0, then w = fl(w + g(s)), s ascending: one f32 a stored row;
//   pair term   : b = the canonical distance (L2) or inner product (IP, cosine) of q to c_l, as the coarse quantiser ranks the lists;
//   row score   : acc = +0, then acc = fl(acc + P[s][code[s]]), s ascending; dis = fl(fl(b + w) - fl(2 * acc)) (L2), fl(b + acc) (IP).

/// P[q][s * ksub + j] for the nq padded queries (ld floats each) of a round.  grid: (ceil(nq / TQ), ceil(m / SPP)); thread (sub, j)
/// of a block as in the scan's table build, its codebook entry read once for the block's TQ queries.  Queries beyond nq repeat the
/// last one and are not written (nq >= 1); s < m keeps the codebook load and the table index inside their arrays.
template <int BITS, int TQ>
static __global__ __launch_bounds__(BLOCK) void pq_query_table_kernel(const float * Q, const float * cbT, uint32_t nq, uint32_t ld, uint32_t m,
                                                                      uint32_t dsub, float * P)
{
    constexpr uint32_t KSUB = 1u << BITS, SPP = BLOCK / KSUB;
    const uint32_t s = blockIdx.y * SPP + threadIdx.x / KSUB, j = threadIdx.x % KSUB;
    if (s >= m)
        return;
    const uint32_t q0 = blockIdx.x * TQ, gw = pq_cb_stride<BITS>(s, m), c0 = s * dsub;
    const float * cb = cbT + pq_cb_index<BITS>(s, 0, j, m, dsub);
    const float * q[TQ];
    float e[TQ];
#pragma unroll
    for (int t = 0; t < TQ; t++)
    {
        q[t] = Q + (size_t)min(q0 + t, nq - 1) * ld + c0;
        e[t] = 0.f;
    }
    for (uint32_t u = 0; u < dsub; u++)
    {
        const float v = cb[(size_t)u * gw];
#pragma unroll
        for (int t = 0; t < TQ; t++)
            e[t] = __fadd_rn(e[t], __fmul_rn(q[t][u], v));
    }
#pragma unroll
    for (int t = 0; t < TQ; t++)
        if (q0 + t < nq)
            P[((size_t)(q0 + t) * m + s) * KSUB + j] = e[t];
}

/// w[r] for the n list-major rows of an L2 index, one thread a row: its list by bisection of list_off (the last l with
/// list_off[l] <= r: empty lists share their offset with the next one), its codes from the stored words (pq_code_word).
template <int BITS>
static __global__ void pq_row_terms_kernel(const uint32_t * codes, const int64_t * list_off, const float * C, const float * cbT, size_t n,
                                           uint32_t nlist, uint32_t ld, uint32_t m, uint32_t dsub, uint32_t mw, float * w)
{
    constexpr uint32_t KSUB = 1u << BITS, CPW = 32 / BITS;
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n)
        return;
    uint32_t lo = 0, hi = nlist; // list_off[lo] <= r < list_off[hi] (list_off[0] = 0, list_off[nlist] = n)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (list_off[mid] <= (int64_t)r)
            lo = mid;
        else
            hi = mid;
    }
    const float * c = C + (size_t)lo * ld;
    float acc = 0.f;
    uint32_t word = 0;
    for (uint32_t s = 0; s < m; s++)
    {
        if (s % CPW == 0)
            word = codes[pq_code_word(r, s / CPW, mw)];
        const uint32_t code = (word >> (BITS * (s % CPW))) & (KSUB - 1), gw = pq_cb_stride<BITS>(s, m);
        const float * cb = cbT + pq_cb_index<BITS>(s, 0, code, m, dsub);
        float g = 0.f;
        for (uint32_t t = 0; t < dsub; t++)
        {
            const float v = cb[(size_t)t * gw], ct = c[s * dsub + t];
            g = __fadd_rn(g, __fmul_rn(v, __fadd_rn(__fadd_rn(ct, ct), v)));
        }
        acc = __fadd_rn(acc, g);
    }
    w[r] = acc;
}

// ------------------------------------------------------------------------------------------ list scan

struct PqIvfParams
{
    const uint32_t * codes;  // stored codes (pq_code_word)
    const uint32_t * labels; // label of row r
    const uint64_t * alive;  // nullable filter bitmap over labels
    const float * Q;         // queries, ld floats each (zero padded)
    const float * cent;      // [nlist][ld]
    const float * cbT;       // the codebooks in the order of pq_cb_index
    uint64_t * partial;      // [(pair * seg_max + segment)][k]
    uint32_t nbits, ld, dim, m, dsub, mw, k;
    uint32_t nprobe;         // probes per query (pair i = q * nprobe + p)
    uint32_t nlist, rows_per_block, seg_max;
    uint32_t tables_only;    // measurement: the row loop is skipped (every partial list comes out empty)
    const int64_t * list_off; // [nlist + 1]
    const uint32_t * pair_off, * work_off, * pairs; // the plan (IvfPlanParams)
    // the query-table form (FORM 1) only
    const float * qtab;   // [query of the round][s * ksub + j]: pq_query_table_kernel's P
    const float * pair_b; // [query][probe], indexed like pairs: the canonical distance / inner product of the query to the probe's centroid
    const float * row_w;  // [row]: pq_row_terms_kernel's w (L2 indexes)
    const uint64_t * after; // AFTER 1 only: [query of the round] continuation keys (search in rounds, coded_ivf.hpp)
};

/// LDS bytes of a scan block: the tile's look-up tables (4 * ksub bytes per query and sub-space), its queries, the list's centroid,
/// and the merge lists.  The query-table form stages no query and no centroid: tables, merge lists and the tile's T pair terms.
inline size_t pq_lds_bytes(size_t bits, uint32_t T, uint32_t m, uint32_t ld, uint32_t k, int form = 0)
{
    const size_t tables = (size_t)T * m * ((size_t)4 << bits), merge = (size_t)T * 5 * k * 8;
    return form ? tables + merge + (size_t)T * 4 : tables + (size_t)(T + 1) * ld * 4 + merge;
}

/// grid: any size; slot -> work item (list, query tile, row segment) as in sq_ivf_scan_kernel.  dynamic LDS: pq_lds_bytes(BITS, T, m, ld, k).
/// Tables and queries keep the T queries of the tile innermost: lut[(s * KSUB + j) * T + t], qs[c * T + t] -- one LDS read serves the
/// whole tile (T <= 4) or half of it.  BITS enters in three places only: the size of a table, which (sub-space, entry) pair a thread
/// of the table build takes (and where its codebook entry is), and how a code comes out of a word.
/// FORM 1 (query_tables=1; dynamic LDS pq_lds_bytes(BITS, T, m, ld, k, 1)): the prologue stages no query and no centroid and computes
/// nothing -- it copies the table P of each tile query (pq_query_table_kernel) into lut and the pairs' terms b into bs; the row loop
/// sums the same look-ups and the row's score is fl(fl(b + w[r]) - fl(2 * acc)) (L2) or fl(b + acc) (IP, cosine).
/// AFTER 1: as in sq_ivf_scan_kernel -- a row is offered to tile query t only if its key is strictly greater than
/// a.after[query of t], read once per work item into scalar registers.  AFTER 0 never reads a.after.
template <int BITS, int METRIC, int T, int R, int FORM = 0, int AFTER = 0>
__global__ __launch_bounds__(BLOCK) void pq_ivf_scan_kernel(const PqIvfParams a)
{
    constexpr uint32_t KSUB = 1u << BITS;  // entries of a table
    constexpr int CPW = 32 / BITS;         // codes per word
    constexpr uint32_t SPP = BLOCK / KSUB; // sub-spaces per pass of the table build: 1 or 16
    const uint32_t ld = a.ld, k = a.k, m = a.m, dsub = a.dsub, mw = a.mw;
    float * lut = reinterpret_cast<float *>(msvs_smem); // [m][KSUB][T]
    float * qs = lut + (size_t)m * KSUB * T;            // [ld][T] (FORM 0)
    float * cs = qs + (size_t)ld * T;                   // [ld] centroid of the item's list (FORM 0)
    uint64_t * lds_merge = reinterpret_cast<uint64_t *>(FORM ? qs : cs + ld); // (the tables are a multiple of 64 bytes)
    float * bs = reinterpret_cast<float *>(lds_merge + (size_t)T * 5 * k); // [T] the pairs' terms (FORM 1)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nu = (mw + 3) >> 2; // units of four code words per row

    const uint32_t total = a.work_off[a.nlist];
    const uint32_t per_xcd = (total + 7) / 8;
    for (uint32_t slot = blockIdx.x; slot < 8 * per_xcd; slot += gridDim.x)
    {
        const uint32_t w = ivf_slot_item(slot, per_xcd);
        if (w >= total)
            continue;
        const IvfWorkItem it = ivf_work_item<T>(w, a.work_off, a.pair_off, a.list_off, a.nlist, a.rows_per_block);
        const uint32_t l = it.list, seg = it.seg, row_begin = it.row_begin, row_end = it.row_end;
        uint64_t * out[T];
        uint64_t floor_key[T];
        __syncthreads(); // the previous item is done with the LDS
#pragma unroll
        for (int t = 0; t < T; t++)
        {
            const uint32_t pi = min(it.pair_begin + t, it.pair_end - 1); // short tiles repeat their last pair (same slot, same values)
            const uint32_t qp = a.pairs[pi];
            out[t] = a.partial + ((size_t)qp * a.seg_max + seg) * k;
            floor_key[t] = AFTER ? uniform_key(a.after[qp / a.nprobe]) : 0;
            if (FORM)
            {
                // the query's table, four entries a load (m * KSUB is a multiple of 16, a table is 64-byte aligned): i4 < m * KSUB / 4
                // keeps the load inside the query's table and the stores below m * KSUB * T
                const float4 * src = reinterpret_cast<const float4 *>(a.qtab + (size_t)(qp / a.nprobe) * m * KSUB);
                for (uint32_t i4 = tid; i4 < m * (KSUB / 4); i4 += BLOCK)
                {
                    const float4 v = src[i4];
                    float * dst = lut + (size_t)i4 * 4 * T + t;
                    dst[0] = v.x;
                    dst[T] = v.y;
                    dst[2 * T] = v.z;
                    dst[3 * T] = v.w;
                }
                if (tid == 0)
                    bs[t] = a.pair_b[qp];
                continue;
            }
            const float * src = a.Q + (size_t)(qp / a.nprobe) * ld;
            for (uint32_t c = tid; c < ld; c += BLOCK)
                qs[c * T + t] = src[c];
        }
        if (!FORM)
            for (uint32_t c = tid; c < ld; c += BLOCK)
                cs[c] = a.cent[(size_t)l * ld + c];
        __syncthreads();

        // the tables: thread (sub, j) of a pass scores entry j of sub-space s0 + sub against the tile's queries (cb[s][j] read once for
        // all T).  Where a pass holds several sub-spaces the last one may be partial: s < m keeps both the codebook load and the table
        // index (s * KSUB + j) * T + t < m * KSUB * T inside their arrays
        for (uint32_t s0 = 0; !FORM && s0 < m; s0 += SPP)
        {
            const uint32_t s = SPP == 1 ? s0 : s0 + tid / KSUB, j = SPP == 1 ? tid : tid % KSUB;
            if (SPP == 1 || s < m)
            {
                // (8 bits: pq_cb_index<8>(s, 0, j, m, dsub), spelled out: see there)
                const float * cb = BITS == 8 ? a.cbT + (size_t)s * dsub * 256 + j : a.cbT + pq_cb_index<BITS>(s, 0, j, m, dsub);
                const uint32_t gw = pq_cb_stride<BITS>(s, m), c0 = s * dsub;
                float e[T];
#pragma unroll
                for (int t = 0; t < T; t++)
                    e[t] = 0.f;
                for (uint32_t u = 0; u < dsub; u++)
                {
                    const float xh = __fadd_rn(cs[c0 + u], cb[(size_t)u * gw]);
                    const float * q = qs + (size_t)(c0 + u) * T;
#pragma unroll
                    for (int t = 0; t < T; t++)
                    {
                        if (METRIC == M_L2)
                        {
                            const float df = __fsub_rn(q[t], xh);
                            e[t] = __fadd_rn(e[t], __fmul_rn(df, df));
                        }
                        else
                            e[t] = __fadd_rn(e[t], __fmul_rn(q[t], xh));
                    }
                }
                float * dst = lut + ((size_t)s * KSUB + j) * T;
#pragma unroll
                for (int t = 0; t < T; t++)
                    dst[t] = e[t];
            }
        }
        __syncthreads();

        WaveTopK<R> top[T];
#pragma unroll
        for (int t = 0; t < T; t++)
            top[t].init();

        // unit u (code words 4u .. 4u + 3, 0 beyond the row's mw words: those are never loaded) of row r
        auto load_unit = [&](uint32_t r, uint32_t u) {
            const uint32_t * p = a.codes + pq_code_word(r, u * 4, mw);
            const uint32_t left = mw - u * 4;
            uint4 v;
            v.x = p[0];
            v.y = left > 1 ? p[64] : 0u;
            v.z = left > 2 ? p[128] : 0u;
            v.w = left > 3 ? p[192] : 0u;
            return v;
        };

        if (!a.tables_only && row_begin < row_end)
        {
            uint4 wnext = load_unit(min(row_begin + tid, row_end - 1), 0);
            for (uint32_t base = row_begin; base < row_end; base += BLOCK)
            {
                const uint32_t r = base + tid;
                const bool rv = r < row_end;
                const uint32_t rc = min(r, row_end - 1); // lanes beyond the segment repeat its last row and offer nothing
                float dis[T];
#pragma unroll
                for (int t = 0; t < T; t++)
                    dis[t] = 0.f;
                for (uint32_t u = 0; u < nu; u++)
                {
                    const uint4 cw = wnext;
                    // the next unit's codes are on their way while this one is looked up: the row's next unit, or the next step's first
                    if (u + 1 < nu)
                        wnext = load_unit(rc, u + 1);
                    else if (base + BLOCK < row_end)
                        wnext = load_unit(min(r + BLOCK, row_end - 1), 0);
                    const uint32_t words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
                    for (int e = 0; e < 4; e++)
                    {
#pragma unroll
                        for (int b = 0; b < CPW; b++)
                        {
                            const uint32_t s = u * 4 * CPW + e * CPW + b;
                            if (s < m) // (pad codes and the words that were not loaded)
                            {
                                const uint32_t code = (words[e] >> (BITS * b)) & (KSUB - 1);
                                const float * src = lut + ((size_t)s * KSUB + code) * T;
#pragma unroll
                                for (int t = 0; t < T; t++)
                                    dis[t] = __fadd_rn(dis[t], src[t]);
                            }
                        }
                    }
                }
                uint32_t id = 0;
                bool ok = rv;
                if (ok)
                {
                    id = a.labels[r];
                    if (a.alive)
                        ok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
                }
                if (FORM)
                {
                    const float w = METRIC == M_L2 ? a.row_w[rc] : 0.f;
#pragma unroll
                    for (int t = 0; t < T; t++)
                        dis[t] = METRIC == M_L2 ? __fsub_rn(__fadd_rn(bs[t], w), __fmul_rn(2.f, dis[t])) : __fadd_rn(bs[t], dis[t]);
                }
#pragma unroll
                for (int t = 0; t < T; t++)
                {
                    uint64_t key = ok ? make_key<METRIC>(dis[t], id) : KEY_NONE;
                    if (AFTER)
                        key = key > floor_key[t] ? key : KEY_NONE;
                    top[t].offer(key, k, lane);
                }
            }
        }

        tile_rank_merge<T, R>(top, lds_merge, out, k); // (no barrier in front: the row loop reads the tables, not lds_merge)
    }
}

}
