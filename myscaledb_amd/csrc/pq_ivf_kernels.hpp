// pq_ivf_kernels.hpp -- device code of the IVFPQ index (pq_index.hip): m code bytes and a label are ALL the index keeps of a row.
//
//   codebooks : m sub-quantisers of 256 entries, cb[s][j] of dsub = dim / m floats; on the device TRANSPOSED, cbT[s][t][j], so that
//               thread j of a block reads entry j and a wavefront's loads are contiguous;
//   decode    : x^[s * dsub + t] = fl(c_l[s * dsub + t] + cb[s][code[s]][t]);
//   sub-score : e(s, j) = sum over t ascending, sequential from +0, of fl(fl(q_t - x^_t)^2) (L2) or fl(q_t * x^_t) (IP, cosine);
//   encode    : code[s] = argmin_j of the L2 sub-score of the stored row against x^ (key = ordered word of e, then j; NaN never wins);
//   distance  : dis = +0, then dis = fl(dis + e(s, code[s])) for s = 0 .. m - 1: the ADC sum over a per-(query, list) table.
//
// Stored codes: a row is mw = ceil(m / 4) 32-bit words (code s in byte s % 4 of word s / 4, zero padded); the rows, list-major, are
// kept in blocks of 64 TRANSPOSED: word w of row r is codes[((r / 64) * mw + w) * 64 + r % 64].  The scan takes one row per lane, so a
// wavefront's load of word w is 256 contiguous bytes (two pieces where its 64 rows straddle a block).  pq_code_word is the map.
//
// The 4-bit form (bit_size = 4; the pq4_* names at the end of this file): the same definitions with 16 entries per sub-quantiser.  A
// row is mw = ceil(m / 8) words, code s in bits 4 * (s % 8) .. + 3 of word s / 8, pad nibbles 0, in the same transposed blocks; the
// codebooks sit on the device in groups of four sub-spaces (pq4_cb_index); the tables are 64 * m bytes per query, so tiles of up to
// 8 queries fit the LDS at every m <= 256.  The 8-bit kernels above it are untouched by it.
#pragma once

#include "scan_kernels.hpp"

namespace msvs
{

// The whole LDS of a CU: the look-up tables are T * m KiB.  pq_fits (pq_index.hip) admits shapes whose T = 1 image is EXACTLY this
// (dim 2816, m 128), so pq_ivf_scan_kernel and everything it calls (tile_rank_merge, WaveTopK) must keep every LDS byte inside the
// dynamic image that pq_lds_bytes counts: a static __shared__ variable anywhere on that path makes such an index fail at launch
// (pq_launch checks the compiled kernel's static LDS once and refuses to run rather than let that happen unnoticed).
constexpr size_t PQ_LDS_BUDGET = 160 * 1024;

/// index of word w of (list-major) row r in the stored codes, rows of mw words
__host__ __device__ inline size_t pq_code_word(size_t r, uint32_t w, uint32_t mw) { return ((r >> 6) * mw + w) * 64 + (r & 63); }

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

__device__ __forceinline__ uint64_t pq_wave_min(uint64_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
    {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        v = other < v ? other : v;
    }
    return v;
}

/// codes[r][s] (rows of mp = 4 * mw bytes, bytes m .. mp - 1 untouched) = code of sub-space s of row r against the centroid of list[r].
/// A block takes rows_per_block rows, thread j codebook entry j; the row and its centroid are staged in LDS (dynamic: 2 * d floats);
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
            const float * cb = cbT + (size_t)s * dsub * 256 + tid;
            const uint32_t c0 = s * dsub;
            float e = 0.f;
            for (uint32_t t = 0; t < dsub; t++)
            {
                const float xh = __fadd_rn(cs[c0 + t], cb[(size_t)t * 256]);
                const float df = __fsub_rn(xs[c0 + t], xh);
                e = __fadd_rn(e, __fmul_rn(df, df));
            }
            uint64_t key = e == e ? ((uint64_t)f2ord(e) << 32 | tid) : KEY_NONE; // (a NaN score never wins)
            key = pq_wave_min(key);
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

/// dst[pq_code_word(pos[r], w)] = src[r][w] for n staged rows of mw words (the staged chunks into their list-major places)
static __global__ void pq_scatter_rows_kernel(const uint32_t * src, uint32_t * dst, const uint32_t * pos, size_t n, uint32_t mw)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * mw)
        return;
    const size_t r = i / mw;
    dst[pq_code_word(pos[r], (uint32_t)(i - r * mw), mw)] = src[i];
}

// ------------------------------------------------------------------------------------------ list scan

struct PqIvfParams
{
    const uint32_t * codes;  // stored codes (pq_code_word)
    const uint32_t * labels; // label of row r
    const uint64_t * alive;  // nullable filter bitmap over labels
    const float * Q;         // queries, ld floats each (zero padded)
    const float * cent;      // [nlist][ld]
    const float * cbT;       // [m][dsub][256]
    uint64_t * partial;      // [(pair * seg_max + segment)][k]
    uint32_t nbits, ld, dim, m, dsub, mw, k;
    uint32_t nprobe;         // probes per query (pair i = q * nprobe + p)
    uint32_t nlist, rows_per_block, seg_max;
    uint32_t tables_only;    // measurement: the row loop is skipped (every partial list comes out empty)
    const int64_t * list_off; // [nlist + 1]
    const uint32_t * pair_off, * work_off, * pairs; // the plan (IvfPlanParams)
};

/// LDS bytes of a scan block: the tile's look-up tables, its queries, the list's centroid, and the merge lists.
inline size_t pq_lds_bytes(uint32_t T, uint32_t m, uint32_t ld, uint32_t k)
{
    return (size_t)T * m * 1024 + (size_t)(T + 1) * ld * 4 + (size_t)T * 5 * k * 8;
}

/// grid: any size; slot -> work item (list, query tile, row segment) as in sq_ivf_scan_kernel.  dynamic LDS: pq_lds_bytes(T, m, ld, k).
/// Tables and queries keep the T queries of the tile innermost: lut[(s * 256 + j) * T + t], qs[c * T + t] -- one LDS read serves the
/// whole tile (T <= 4) or half of it.
template <int METRIC, int T, int R>
__global__ __launch_bounds__(BLOCK) void pq_ivf_scan_kernel(const PqIvfParams a)
{
    const uint32_t ld = a.ld, k = a.k, m = a.m, dsub = a.dsub, mw = a.mw;
    float * lut = reinterpret_cast<float *>(msvs_smem); // [m][256][T]
    float * qs = lut + (size_t)m * 256 * T;             // [ld][T]
    float * cs = qs + (size_t)ld * T;                   // [ld] centroid of the item's list
    uint64_t * lds_merge = reinterpret_cast<uint64_t *>(cs + ld);
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
        __syncthreads(); // the previous item is done with the LDS
#pragma unroll
        for (int t = 0; t < T; t++)
        {
            const uint32_t pi = min(it.pair_begin + t, it.pair_end - 1); // short tiles repeat their last pair (same slot, same values)
            const uint32_t qp = a.pairs[pi];
            out[t] = a.partial + ((size_t)qp * a.seg_max + seg) * k;
            const float * src = a.Q + (size_t)(qp / a.nprobe) * ld;
            for (uint32_t c = tid; c < ld; c += BLOCK)
                qs[c * T + t] = src[c];
        }
        for (uint32_t c = tid; c < ld; c += BLOCK)
            cs[c] = a.cent[(size_t)l * ld + c];
        __syncthreads();

        // the tables: thread j scores codebook entry j of every sub-space against the tile's queries (cb[s][j] read once for all T)
        for (uint32_t s = 0; s < m; s++)
        {
            const float * cb = a.cbT + (size_t)s * dsub * 256 + tid;
            const uint32_t c0 = s * dsub;
            float e[T];
#pragma unroll
            for (int t = 0; t < T; t++)
                e[t] = 0.f;
            for (uint32_t u = 0; u < dsub; u++)
            {
                const float xh = __fadd_rn(cs[c0 + u], cb[(size_t)u * 256]);
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
            float * dst = lut + ((size_t)s * 256 + tid) * T;
#pragma unroll
            for (int t = 0; t < T; t++)
                dst[t] = e[t];
        }
        __syncthreads();

        WaveTopK<R> top[T];
#pragma unroll
        for (int t = 0; t < T; t++)
            top[t].init();

        // unit u (code words 4u .. 4u + 3, 0 beyond the row's mw words) of row r
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
                const uint32_t rc = min(r, row_end - 1);
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
                        for (int b = 0; b < 4; b++)
                        {
                            const uint32_t s = u * 16 + e * 4 + b;
                            if (s < m)
                            {
                                const uint32_t code = (words[e] >> (8 * b)) & 255u;
                                const float * src = lut + ((size_t)s * 256 + code) * T;
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
#pragma unroll
                for (int t = 0; t < T; t++)
                    top[t].offer(ok ? make_key<METRIC>(dis[t], id) : KEY_NONE, k, lane);
            }
        }

        tile_rank_merge<T, R>(top, lds_merge, out, k); // (no barrier in front: the row loop reads the tables, not lds_merge)
    }
}

// ------------------------------------------------------------------------------------------ the 4-bit form

/// floats between the entries u and u + 1 of one codebook entry in the device copy of the 16-entry codebooks: 16 for every
/// sub-space of the group of four that s belongs to (the last group has m % 4 of them when 4 does not divide m)
__host__ __device__ inline uint32_t pq4_cb_stride(uint32_t s, uint32_t m) { return (m - (s & ~3u) < 4u ? m - (s & ~3u) : 4u) * 16; }

/// index of cb[s][j][u] in that copy: [group of four sub-spaces][u][sub-space in the group][j], 16 * dim floats in all, no padding.
/// The 64 lanes of a wavefront that build tables are (4 consecutive sub-spaces) x (16 entries), so their load at step u is 256
/// contiguous bytes; the 16 lanes that encode one row read 64 contiguous bytes.
__host__ __device__ inline size_t pq4_cb_index(uint32_t s, uint32_t u, uint32_t j, uint32_t m, uint32_t dsub)
{
    return (size_t)(s >> 2) * dsub * 64 + (size_t)u * pq4_cb_stride(s, m) + (s & 3) * 16 + j;
}

/// LDS bytes of a 4-bit scan block: 16-entry tables, the tile's queries, the list's centroid, the merge lists.
inline size_t pq4_lds_bytes(uint32_t T, uint32_t m, uint32_t ld, uint32_t k)
{
    return (size_t)T * m * 64 + (size_t)(T + 1) * ld * 4 + (size_t)T * 5 * k * 8;
}

/// the minimum over each group of 16 consecutive lanes, in all of them
__device__ __forceinline__ uint64_t pq4_group_min(uint64_t v)
{
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1)
    {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
        const uint64_t other = (uint64_t)hi << 32 | lo;
        v = other < v ? other : v;
    }
    return v;
}

/// pq_encode_kernel with 16 entries: codes[r][s / 2] (rows of mp = 4 * mw bytes; bytes ceil(m / 2) .. mp - 1 untouched) holds code s in
/// its low (s even) or high nibble.  A block takes 16 rows, 16 lanes a row, lane j entry j (cb4: pq4_cb_index); the argmin over the
/// key (ordered word of e, j) is four shuffles.  Lane 0 of a row collects two codes and writes the whole byte: no byte has two writers.
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
        const float * cb = cb4 + pq4_cb_index(s, 0, j, m, dsub);
        const uint32_t gw = pq4_cb_stride(s, m), c0 = s * dsub;
        float e = 0.f;
        for (uint32_t t = 0; t < dsub; t++)
        {
            const float xh = __fadd_rn(c[c0 + t], cb[(size_t)t * gw]);
            const float df = __fsub_rn(x[c0 + t], xh);
            e = __fadd_rn(e, __fmul_rn(df, df));
        }
        const uint64_t best = pq4_group_min(e == e ? ((uint64_t)f2ord(e) << 32 | j) : KEY_NONE); // (a NaN score never wins)
        const uint32_t code = best == KEY_NONE ? 0u : (uint32_t)(best & 15u);
        byte = (s & 1) ? byte | code << 4 : code;
        if (j == 0 && r < n && ((s & 1) || s + 1 == m))
            codes[r * mp + (s >> 1)] = (uint8_t)byte;
    }
}

/// pq_ivf_scan_kernel with 16-entry tables, lut[(s * 16 + j) * T + t]: the same work items, prologue, arithmetic, top-k and merge.
/// dynamic LDS: pq4_lds_bytes(T, m, ld, k); a.cbT is the pq4_cb_index copy, a.mw = ceil(m / 8).
/// The tables are built by (sub-space, entry) pairs, 16 sub-spaces a pass (the last pass is partial when 16 does not divide m); the
/// row loop is one lane per row with eight codes a word.
template <int METRIC, int T, int R>
__global__ __launch_bounds__(BLOCK) void pq4_ivf_scan_kernel(const PqIvfParams a)
{
    const uint32_t ld = a.ld, k = a.k, m = a.m, dsub = a.dsub, mw = a.mw;
    float * lut = reinterpret_cast<float *>(msvs_smem); // [m][16][T]
    float * qs = lut + (size_t)m * 16 * T;              // [ld][T]
    float * cs = qs + (size_t)ld * T;                   // [ld] centroid of the item's list
    uint64_t * lds_merge = reinterpret_cast<uint64_t *>(cs + ld);
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
        __syncthreads(); // the previous item is done with the LDS
#pragma unroll
        for (int t = 0; t < T; t++)
        {
            const uint32_t pi = min(it.pair_begin + t, it.pair_end - 1); // short tiles repeat their last pair (same slot, same values)
            const uint32_t qp = a.pairs[pi];
            out[t] = a.partial + ((size_t)qp * a.seg_max + seg) * k;
            const float * src = a.Q + (size_t)(qp / a.nprobe) * ld;
            for (uint32_t c = tid; c < ld; c += BLOCK)
                qs[c * T + t] = src[c];
        }
        for (uint32_t c = tid; c < ld; c += BLOCK)
            cs[c] = a.cent[(size_t)l * ld + c];
        __syncthreads();

        // the tables: thread (sub, j) of a pass scores entry j of sub-space s0 + sub against the tile's queries; s < m keeps both the
        // codebook load and the table index (s * 16 + j) * T + t < m * 16 * T inside their arrays
        for (uint32_t s0 = 0; s0 < m; s0 += 16)
        {
            const uint32_t s = s0 + (tid >> 4), j = tid & 15;
            if (s < m)
            {
                const float * cb = a.cbT + pq4_cb_index(s, 0, j, m, dsub);
                const uint32_t gw = pq4_cb_stride(s, m), c0 = s * dsub;
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
                float * dst = lut + ((size_t)s * 16 + j) * T;
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
                        for (int b = 0; b < 8; b++)
                        {
                            const uint32_t s = u * 32 + e * 8 + b;
                            if (s < m) // (pad nibbles and the words that were not loaded)
                            {
                                const uint32_t code = (words[e] >> (4 * b)) & 15u;
                                const float * src = lut + ((size_t)s * 16 + code) * T;
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
#pragma unroll
                for (int t = 0; t < T; t++)
                    top[t].offer(ok ? make_key<METRIC>(dis[t], id) : KEY_NONE, k, lane);
            }
        }

        tile_rank_merge<T, R>(top, lds_merge, out, k); // (no barrier in front: the row loop reads the tables, not lds_merge)
    }
}

}
