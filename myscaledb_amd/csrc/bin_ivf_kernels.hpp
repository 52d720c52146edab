// bin_ivf_kernels.hpp -- the partitioned (IVF) form of the binary index: k-majority centroids + list-major rows.
//
// Everything is integer popcounts (bin_kernels.hpp) plus, for Jaccard, the one f32 division of the exact counts:
//   coarse distance : Hamming(query or row, centroid) for BOTH index metrics (as in Faiss' binary IVF);
//   assignment      : the list with the smallest (Hamming distance, list id);
//   probe set       : the first min(nprobe, nlist) lists by (Hamming distance, list id) -- a SET: the order of the probes
//                     changes no result, so the selection writes them in no particular order;
//   list scan       : work items (list, tile of <= T of the queries that probe it, row segment) from the float path's plan
//                     (ivf_hist / ivf_plan_scan / ivf_scatter kernels, scan_kernels.hpp); the tile's queries sit in LDS (in
//                     registers when a lane holds one 16-byte word of the row), the rows are streamed with 16-byte loads, G lanes
//                     per row, so a list's rows come from HBM once per tile instead of once per query; one WaveTopK per query.
#pragma once

#include "bin_kernels.hpp"

namespace msvs
{

__device__ __forceinline__ uint32_t popc_xor4(const uint4 x, const uint4 y)
{
    return __popc(x.x ^ y.x) + __popc(x.y ^ y.y) + __popc(x.z ^ y.z) + __popc(x.w ^ y.w);
}

// ------------------------------------------------------------------------------------------ assign / coarse

struct BinAssignParams
{
    const uint4 * Y; // n rows (or queries), ld16 uint4 each (zero padded)
    const uint4 * C; // nlist centroids, same stride
    uint32_t n, nlist, ld16;
    uint32_t tile;    // centroids per LDS tile (dynamic LDS: tile * ld16 * 16 bytes)
    uint32_t * best;  // nullable [n]: the list with the smallest (distance, list id)
    uint32_t * dist;  // nullable [n][nlist]: every distance (the probe selection's input)
};

/// One row per group of G lanes (the row's 16-byte words dealt round-robin over the group, as in bin_scan_kernel), 256 / G rows
/// per block, grid = ceil(n / (256 / G)) blocks in x (rows never sit on grid.y); the centroids pass through LDS tile by tile.
template <int G>
__global__ __launch_bounds__(BLOCK) void bin_assign_kernel(const BinAssignParams a)
{
    uint4 * cs = reinterpret_cast<uint4 *>(msvs_smem);
    const uint32_t tid = threadIdx.x, grp = tid / G, g = tid % G;
    const size_t row = (size_t)blockIdx.x * (BLOCK / G) + grp;
    const bool rv = row < a.n;
    const uint4 * yrow = a.Y + (rv ? row : (size_t)a.n - 1) * a.ld16;
    const bool one = a.ld16 == G; // a lane holds its only word of the row in registers
    const uint4 y0 = yrow[g < a.ld16 ? g : 0];
    uint64_t best = KEY_NONE;
    for (uint32_t base = 0; base < a.nlist; base += a.tile)
    {
        const uint32_t nt = min(a.tile, a.nlist - base);
        __syncthreads();
        for (uint32_t i = tid; i < nt * a.ld16; i += BLOCK)
            cs[i] = a.C[(size_t)base * a.ld16 + i];
        __syncthreads();
        for (uint32_t j = 0; j < nt; j++)
        {
            const uint4 * c = cs + (size_t)j * a.ld16;
            uint32_t cnt = 0;
            if (one)
                cnt = popc_xor4(y0, c[g]);
            else
                for (uint32_t w = g; w < a.ld16; w += G)
                    cnt += popc_xor4(yrow[w], c[w]);
#pragma unroll
            for (int o = G / 2; o >= 1; o >>= 1)
                cnt += (uint32_t)__shfl_xor((int)cnt, o);
            const uint64_t key = (uint64_t)cnt << 32 | (base + j);
            best = key < best ? key : best;
            if (a.dist && rv && g == 0)
                a.dist[row * a.nlist + base + j] = cnt;
        }
    }
    if (a.best && rv && g == 0)
        a.best[row] = (uint32_t)best;
}

/// Sum over the block of one count per thread (every thread gets it; two barriers).
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t * s4, uint32_t tid)
{
    v = wave_sum_u32(v);
    __syncthreads();
    if ((tid & 63) == 0)
        s4[tid >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

/// One block per query: the P lists with the smallest (distance, list id) out of dist[q][0 .. nlist) -> probes[q][0 .. P), P <= nlist.
/// The distances are small integers (<= max_d): a bisection finds the P-th smallest one, d; every list below d is taken, and the
/// lowest-numbered lists AT d fill the rest.
static __global__ __launch_bounds__(BLOCK) void bin_probe_select_kernel(const uint32_t * dist, uint32_t nlist, uint32_t P, uint32_t max_d,
                                                                        int32_t * probes)
{
    __shared__ uint32_t s4[4];
    __shared__ uint32_t s_lt[4], s_eq[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t * d = dist + (size_t)blockIdx.x * nlist;
    int32_t * out = probes + (size_t)blockIdx.x * P;
    uint32_t lo = 0, hi = max_d; // the smallest value v with #(d <= v) >= P is in [lo, hi]
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi) >> 1;
        uint32_t c = 0;
        for (uint32_t j = tid; j < nlist; j += BLOCK)
            c += d[j] <= mid;
        if (block_sum_u32(c, s4, tid) >= P)
            hi = mid;
        else
            lo = mid + 1;
    }
    uint32_t c = 0;
    for (uint32_t j = tid; j < nlist; j += BLOCK)
        c += d[j] < lo;
    const uint32_t below = block_sum_u32(c, s4, tid);
    uint32_t run_lt = 0, run_eq = 0; // lists below / at the cut among those walked so far (ascending list id)
    for (uint32_t base = 0; base < nlist; base += BLOCK)
    {
        const uint32_t j = base + tid;
        const uint32_t v = j < nlist ? d[j] : 0xffffffffu;
        const bool lt = v < lo, eq = v == lo;
        const uint64_t m_lt = __ballot(lt), m_eq = __ballot(eq);
        __syncthreads();
        if (lane == 0)
        {
            s_lt[wave] = __popcll(m_lt);
            s_eq[wave] = __popcll(m_eq);
        }
        __syncthreads();
        uint32_t p_lt = run_lt, p_eq = run_eq;
        for (uint32_t w = 0; w < 4; w++)
        {
            if (w < wave)
            {
                p_lt += s_lt[w];
                p_eq += s_eq[w];
            }
            run_lt += s_lt[w];
            run_eq += s_eq[w];
        }
        const uint64_t before = ((uint64_t)1 << lane) - 1;
        p_lt += __popcll(m_lt & before);
        p_eq += __popcll(m_eq & before);
        if (lt)
            out[p_lt] = (int32_t)j;
        else if (eq && below + p_eq < P)
            out[below + p_eq] = (int32_t)j;
    }
}

// ------------------------------------------------------------------------------------------ training: vote counts

/// ones[list of row r][bit b] += 1 for every set bit of the row, members[list] += 1: one thread per (row, 32-bit word).
/// words: 32-bit words per row of the PADDED image (ld16 * 4); bits beyond the vector are zero and count nothing.
static __global__ void bin_vote_kernel(const uint32_t * Y, const uint32_t * assign, size_t n, uint32_t words, uint32_t * ones, uint32_t * members)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * words)
        return;
    const size_t r = i / words;
    const uint32_t w = (uint32_t)(i - r * words), l = assign[r];
    if (w == 0)
        atomicAdd(&members[l], 1u);
    uint32_t * o = ones + ((size_t)l * words + w) * 32;
    for (uint32_t m = Y[i]; m; m &= m - 1)
        atomicAdd(&o[__builtin_ctz(m)], 1u);
}

// ------------------------------------------------------------------------------------------ list scan

struct BinIvfParams
{
    const uint4 * Y;         // rows, list-major, ld16 uint4 each
    const uint4 * Q;         // queries, same stride
    const uint64_t * alive;  // nullable filter bitmap over labels
    const uint32_t * labels; // label of row r
    uint32_t nbits, ld16, k;
    uint32_t nprobe;         // probes per query (pair i = q * nprobe + p)
    uint32_t nlist, rows_per_block, seg_max;
    const int64_t * list_off; // [nlist + 1]
    const uint32_t * pair_off, * work_off, * pairs; // the plan (IvfPlanParams)
    uint64_t * partial;       // [pair][seg_max][k], prefilled with KEY_NONE: a (pair, segment) without rows is never written
    const uint64_t * after;   // AFTER 1 only: [query of the round] continuation keys (search in rank rounds, binary.hip)
};

/// grid: any size; slot -> work item as in ivf_batched_scan_kernel (tiles of one list back to back on one XCD).
/// dynamic LDS: T * ld16 * 16 + 5 * k * 8 bytes.  REG: ld16 == G, a lane's word of every query of the tile lives in registers.
/// AFTER 1 (a later round of a search with k > MSVS_MAX_K): a row is offered to tile query t only if its key is strictly greater than
/// a.after[query of t], the last key the query has returned; KEY_NONE there admits nothing.  The tile's floors are read once per work
/// item and are uniform over the workgroup.  AFTER 0 never reads a.after.
template <int METRIC, int G, int T, int R, bool REG, int AFTER = 0>
__global__ __launch_bounds__(BLOCK) void bin_ivf_scan_kernel(const BinIvfParams a)
{
    uint4 * qs = reinterpret_cast<uint4 *>(msvs_smem);
    uint64_t * lds_merge = reinterpret_cast<uint64_t *>(msvs_smem + (size_t)T * a.ld16 * 16);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = a.k;
    constexpr uint32_t RPW = 64 / G;
    const uint32_t grp = lane / G, g = lane % G;
    const uint32_t total = a.work_off[a.nlist];
    const uint32_t per_xcd = (total + 7) / 8;
    for (uint32_t s = blockIdx.x; s < 8 * per_xcd; s += gridDim.x)
    {
        const uint32_t w = ivf_slot_item(s, per_xcd);
        if (w >= total)
            continue;
        const IvfWorkItem it = ivf_work_item<T>(w, a.work_off, a.pair_off, a.list_off, a.nlist, a.rows_per_block);
        const uint32_t seg = it.seg, pb = it.pair_begin, row_begin = it.row_begin, row_end = it.row_end;
        const uint32_t nt = min((uint32_t)T, it.pair_end - pb); // queries of this tile (>= 1)
        __syncthreads(); // the previous item is done with the LDS
        for (uint32_t i = tid; i < nt * a.ld16; i += BLOCK)
        {
            const uint32_t t = i / a.ld16, c = i - t * a.ld16;
            qs[i] = a.Q[(size_t)(a.pairs[pb + t] / a.nprobe) * a.ld16 + c];
        }
        __syncthreads();
        uint64_t floor_key[AFTER ? T : 1];
        if (AFTER)
        {
#pragma unroll
            for (int t = 0; t < T; t++) // (short tiles repeat their last query: its slot is never offered to)
                floor_key[AFTER ? t : 0] = uniform_key(a.after[a.pairs[pb + min((uint32_t)t, nt - 1)] / a.nprobe]);
        }
        uint4 xq[REG ? T : 1];
        if (REG)
        {
#pragma unroll
            for (int t = 0; t < T; t++)
                xq[REG ? t : 0] = qs[(size_t)((uint32_t)t < nt ? t : 0) * a.ld16 + g];
        }
        WaveTopK<R> top[T];
#pragma unroll
        for (int t = 0; t < T; t++)
            top[t].init();
        uint32_t base = row_begin + wave * RPW;
        uint4 ynext = make_uint4(0, 0, 0, 0);
        if (REG && base < row_end)
            ynext = a.Y[(size_t)min(base + grp, row_end - 1) * a.ld16 + g];
        for (; base < row_end; base += 4 * RPW)
        {
            const uint32_t r = base + grp;
            const bool rv = r < row_end;
            const uint4 * yrow = a.Y + (size_t)(rv ? r : row_end - 1) * a.ld16;
            uint32_t c0[T], c1[T]; // Hamming: c0 = xor count; Jaccard: c0 = and count, c1 = or count
#pragma unroll
            for (int t = 0; t < T; t++)
                c0[t] = c1[t] = 0;
            if (REG)
            {
                const uint4 y = ynext;
                if (base + 4 * RPW < row_end) // the next step's word is on its way while this one is counted and offered
                    ynext = a.Y[(size_t)min(base + 4 * RPW + grp, row_end - 1) * a.ld16 + g];
#pragma unroll
                for (int t = 0; t < T; t++)
                {
                    const uint4 x = xq[REG ? t : 0];
                    if (METRIC == B_HAMMING)
                        c0[t] = popc_xor4(x, y);
                    else
                    {
                        c0[t] = __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                        c1[t] = __popc(x.x | y.x) + __popc(x.y | y.y) + __popc(x.z | y.z) + __popc(x.w | y.w);
                    }
                }
            }
            else
            {
                for (uint32_t c = g; c < a.ld16; c += G)
                {
                    const uint4 y = yrow[c];
#pragma unroll
                    for (int t = 0; t < T; t++)
                        if ((uint32_t)t < nt)
                        {
                            const uint4 x = qs[(size_t)t * a.ld16 + c];
                            if (METRIC == B_HAMMING)
                                c0[t] += popc_xor4(x, y);
                            else
                            {
                                c0[t] += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                                c1[t] += __popc(x.x | y.x) + __popc(x.y | y.y) + __popc(x.z | y.z) + __popc(x.w | y.w);
                            }
                        }
                }
            }
            bool ok = rv && g == 0;
            const uint32_t id = a.labels[rv ? r : row_end - 1];
            if (ok && a.alive)
                ok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
#pragma unroll
            for (int t = 0; t < T; t++)
                if ((uint32_t)t < nt)
                {
                    uint32_t x0 = c0[t], x1 = c1[t];
#pragma unroll
                    for (int o = G / 2; o >= 1; o >>= 1)
                    {
                        x0 += (uint32_t)__shfl_xor((int)x0, o);
                        if (METRIC == B_JACCARD)
                            x1 += (uint32_t)__shfl_xor((int)x1, o);
                    }
                    const float v = METRIC == B_HAMMING ? (float)x0 : (x1 == 0 ? 1.0f : __fdiv_rn((float)(x1 - x0), (float)x1));
                    uint64_t key = ok ? make_key<M_L2>(v, id) : KEY_NONE;
                    if (AFTER)
                        key = key > floor_key[AFTER ? t : 0] ? key : KEY_NONE;
                    top[t].offer(key, k, lane);
                }
        }
        uint64_t * merged = lds_merge + 4 * k;
#pragma unroll
        for (int t = 0; t < T; t++)
            if ((uint32_t)t < nt)
            {
                top[t].store(lds_merge + wave * k, k, lane);
                __syncthreads();
                block_rank_merge(lds_merge, k, merged, k, tid);
                uint64_t * out = a.partial + ((size_t)a.pairs[pb + t] * a.seg_max + seg) * k;
                for (uint32_t e = tid; e < k; e += BLOCK)
                    out[e] = merged[e];
                __syncthreads(); // the next query's lists overwrite the stage
            }
    }
}

}
