// sq_cand_kernels.hpp -- device code of the IVFSQ candidate search (sq_candidates.hip; definition: include/msvs.h):
// an exact int8 matrix-core pass over the stored 8-bit codes picks kc candidates per query, a canonical re-rank of those codes
// gives the k results with search's own numbers.
//
//   prepare : sq_cand_prep_kernel      E_row = fl(cip(e, e) + fl(2 cip(c_l, e))) per stored row (L2), e the decode's inner term;
//   round   : sq_query_image_kernel    per query: u = q o step quantised to 15 bits, split into two int8 planes IN THE STORED BYTE
//                                      ORDER (sq_stored_pos), then Qo = cip(q, o) and the scale D;
//             sq_cand_scan_kernel      per (list, tile of queries, row segment): S = 128 sum h s + sum l s by v_mfma_i32_32x32x32_i8
//                                      (s = code - 128: one XOR per four codes; the stored row IS the A operand, the image the B
//                                      operand -- a dot product does not care about the permutation of K both share), the score a,
//                                      the best kc keys (a, position) of the item into the plan's partial lists;
//             sq_cand_rerank_kernel    per query: its kc merged candidates decoded and scored with the list scan's arithmetic
//                                      (sq_ivf_kernels.hpp: the same columns per lane in the same order), ranked by (distance, label).
//
// A query's record (global and LDS alike): ld bytes of h, ld bytes of l, then Qo, D as floats and 8 bytes of padding: 2 ld + 16
// bytes.  The odd 16 bytes also take consecutive queries' 16-byte fragments to different LDS banks.
#pragma once

#include "../../include/msvs.h"
#include "scan_kernels.hpp"
#include "sq_layout.hpp"

namespace msvs
{

typedef int sqc_i32x4 __attribute__((ext_vector_type(4)));
typedef int sqc_i32x16 __attribute__((ext_vector_type(16)));

constexpr float SQC_WMAX = 16256.f;   // 127 * 128: |w| <= SQC_WMAX, so h = floor(w / 128) is in [-127, 127]
constexpr uint32_t SQC_GROUP = 128;   // rows a block scores between two looks at its buffers: 32 per wavefront

/// bytes of a query's record
MSVS_HD inline size_t sqc_record_bytes(uint32_t ld) { return 2 * (size_t)ld + 16; }
/// keys of a query's buffer in the scan: kc kept + a group's worth of new ones, in whole 64s (a lane ranks CAP / 64 of them)
MSVS_HD inline uint32_t sqc_cap(uint32_t kc) { return (kc + SQC_GROUP + 63) / 64 * 64; }
/// LDS bytes of a scan block: TQ records, TQ buffers, and per query: count, threshold, pair, base
inline size_t sqc_lds_bytes(uint32_t TQ, uint32_t ld, uint32_t kc) { return TQ * (sqc_record_bytes(ld) + (size_t)sqc_cap(kc) * 8 + 24); }
constexpr size_t SQC_LDS_MAX = 160 * 1024;

/// The lane's columns of a stored 8-bit row in the list scan's order: f(col, w) for the float4 columns col = g, g + 16, ... (ascending)
/// of lane g of a 16-lane group, w = the column's four codes.  Whole blocks of 256 bytes: one 16-byte load = four columns; the
/// natural-order tail: one word per column.
template <class F>
__device__ __forceinline__ void sqc_for_columns(const uint4 * row, uint32_t ld4, uint32_t g, F f)
{
    const uint32_t nb = ld4 >> 6, tc = ld4 & 63;
    for (uint32_t b = 0; b < nb; b++)
    {
        const uint4 w = row[b * 16 + g];
        f(b * 64 + g, w.x);
        f(b * 64 + g + 16, w.y);
        f(b * 64 + g + 32, w.z);
        f(b * 64 + g + 48, w.w);
    }
    const uint32_t * tail = reinterpret_cast<const uint32_t *>(row) + nb * 64;
#pragma unroll
    for (uint32_t e = 0; e < 4; e++)
        if (g + 16 * e < tc)
            f(nb * 64 + g + 16 * e, tail[g + 16 * e]);
}

/// the decode's inner term of a column: e = fl(vmin + fl(float(code) * step))
__device__ __forceinline__ float4 sqc_inner(uint32_t w, const float4 m, const float4 s)
{
    float4 e;
    e.x = __fadd_rn(m.x, __fmul_rn((float)(w & 255u), s.x));
    e.y = __fadd_rn(m.y, __fmul_rn((float)((w >> 8) & 255u), s.y));
    e.z = __fadd_rn(m.z, __fmul_rn((float)((w >> 16) & 255u), s.z));
    e.w = __fadd_rn(m.w, __fmul_rn((float)(w >> 24), s.w));
    return e;
}

__device__ __forceinline__ void sqc_mac(float4 & s, const float4 a, const float4 b)
{
    s.x = __fadd_rn(s.x, __fmul_rn(a.x, b.x));
    s.y = __fadd_rn(s.y, __fmul_rn(a.y, b.y));
    s.z = __fadd_rn(s.z, __fmul_rn(a.z, b.z));
    s.w = __fadd_rn(s.w, __fmul_rn(a.w, b.w));
}

/// the canonical fold of a 16-lane group's accumulators
__device__ __forceinline__ float sqc_fold(const float4 s) { return row16_tree_sum(__fadd_rn(__fadd_rn(s.x, s.y), __fadd_rn(s.z, s.w))); }

/// the list of row position r: list_off[l] <= r < list_off[l + 1] (r < list_off[nlist])
__device__ __forceinline__ uint32_t sqc_list_of(const int64_t * list_off, uint32_t nlist, uint32_t r)
{
    uint32_t lo = 0, hi = nlist;
    while (hi - lo > 1)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (list_off[mid] <= (int64_t)r)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------ prepare: the row terms

/// erow[r] = fl(cip(e, e) + fl(2 cip(c_l, e))) for the n stored rows; a 16-lane group per row, 16 rows per block
static __global__ __launch_bounds__(BLOCK) void sq_cand_prep_kernel(const uint4 * codes, const float4 * cent, const float4 * vmin,
                                                                   const float4 * step, const int64_t * list_off, uint32_t nlist, uint32_t n,
                                                                   uint32_t ld4, float * erow)
{
    const uint32_t g = threadIdx.x & 15;
    const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= n) // (whole groups leave)
        return;
    const float4 * c = cent + (size_t)sqc_list_of(list_off, nlist, r) * ld4;
    float4 ee = make_float4(0.f, 0.f, 0.f, 0.f), ce = ee;
    sqc_for_columns(codes + (size_t)r * (ld4 >> 2), ld4, g, [&](uint32_t col, uint32_t w) {
        const float4 e = sqc_inner(w, vmin[col], step[col]);
        sqc_mac(ee, e, e);
        sqc_mac(ce, c[col], e);
    });
    const float a = sqc_fold(ee), b = sqc_fold(ce);
    if (g == 0)
        erow[r] = __fadd_rn(a, __fmul_rn(2.f, b));
}

// ------------------------------------------------------------------------------------------ per round: the query images

/// A block per query: its record (see the head of the file) from its padded (and, for cosine, normalised) row.  o_j = fl(vmin_j +
/// fl(128 step_j)) is formed here from the index's own vmin / step (ld floats each, zero padded): no copy of it is kept.
static __global__ __launch_bounds__(BLOCK) void sq_query_image_kernel(const float * Q, const float * vmin, const float * step, uint32_t ld,
                                                                     unsigned char * img)
{
    __shared__ uint32_t mbits;
    const uint32_t tid = threadIdx.x;
    const float * q = Q + (size_t)blockIdx.x * ld;
    unsigned char * rec = img + (size_t)blockIdx.x * sqc_record_bytes(ld);
    if (tid == 0)
        mbits = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t j = tid; j < ld; j += BLOCK)
    {
        const uint32_t b = __float_as_uint(__fmul_rn(q[j], step[j])) & 0x7fffffffu; // (|u|: the bit patterns order as the values; a NaN tops all)
        mine = b > mine ? b : mine;
    }
    atomicMax(&mbits, mine);
    __syncthreads();
    float delta = __fdiv_rn(__uint_as_float(mbits), SQC_WMAX);
    if (!(delta > 0.f && delta < __builtin_inff()))
        delta = 0.f;
    for (uint32_t j = tid; j < ld; j += BLOCK)
    {
        int w = 0;
        if (delta != 0.f)
            w = (int)fminf(fmaxf(rintf(__fdiv_rn(__fmul_rn(q[j], step[j]), delta)), -SQC_WMAX), SQC_WMAX);
        const uint32_t p = sq_stored_pos(j, ld);
        rec[p] = (unsigned char)(signed char)(w >> 7);
        rec[ld + p] = (unsigned char)(w & 127);
    }
    if (tid < WAVE) // Qo = cip(q, o): every 16-lane group of the first wavefront forms it
    {
        const float4 * q4 = reinterpret_cast<const float4 *>(q), * m4 = reinterpret_cast<const float4 *>(vmin),
                     * s4 = reinterpret_cast<const float4 *>(step);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t c = tid & 15; c < ld >> 2; c += 16)
        {
            const float4 m = m4[c], st = s4[c];
            sqc_mac(s, q4[c], make_float4(__fadd_rn(m.x, __fmul_rn(128.f, st.x)), __fadd_rn(m.y, __fmul_rn(128.f, st.y)),
                                          __fadd_rn(m.z, __fmul_rn(128.f, st.z)), __fadd_rn(m.w, __fmul_rn(128.f, st.w))));
        }
        const float qo = sqc_fold(s);
        if (tid == 0)
        {
            float * tailf = reinterpret_cast<float *>(rec + 2 * (size_t)ld);
            tailf[0] = qo;
            tailf[1] = delta;
            tailf[2] = 0.f;
            tailf[3] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------ the candidate scan

struct SqCandParams
{
    const uint4 * codes;     // rows, list-major, ld / 16 uint4 each (stored order)
    const uint32_t * labels; // label of row r
    const uint64_t * alive;  // nullable filter bitmap over labels
    const float * erow;      // L2: the rows' terms (IP: not read)
    const unsigned char * img; // [query of the round] records
    const float * probe_dis; // [pair] the coarse step's canonical distance / inner product to the pair's centroid
    uint64_t * partial;      // [(pair * seg_max + segment)][k]
    uint32_t nbits, ld, k;   // k: the candidates kept, kc
    uint32_t nprobe, nlist, rows_per_block, seg_max;
    const int64_t * list_off;
    const uint32_t * pair_off, * work_off, * pairs; // the plan
    const uint64_t * after;  // (fill_scan_params; never set: one round)
};

/// the key of a candidate: (a, position) ascending = better first, position ascending among equal a; a is compared as a number
/// (-0 = +0); KEY_NONE for a NaN
template <int METRIC>
__device__ __forceinline__ uint64_t sqc_key(float a, uint32_t pos)
{
    if (a != a)
        return KEY_NONE;
    const uint32_t o = f2ord(a == 0.f ? 0.f : a);
    return (uint64_t)(METRIC == M_IP ? ~o : o) << 32 | pos;
}

/// One wavefront sorts query buffer `buf` (c distinct keys, c <= 64 * 6) by rank and keeps the best kc in front; -> the new count.
/// *thr becomes the kc-th key once there are kc.
__device__ __forceinline__ uint32_t sqc_compact(uint64_t * buf, uint32_t c, uint32_t kc, uint64_t * thr, uint32_t lane)
{
    uint64_t key[6];
    uint32_t rank[6];
#pragma unroll
    for (int u = 0; u < 6; u++)
    {
        const uint32_t e = lane + 64 * u;
        key[u] = e < c ? buf[e] : KEY_NONE;
        rank[u] = 0;
    }
    for (uint32_t j = 0; j < c; j++)
    {
        const uint64_t kj = buf[j]; // (one address for the wavefront: a broadcast)
#pragma unroll
        for (int u = 0; u < 6; u++)
            rank[u] += kj < key[u] ? 1u : 0u;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // every read of the old order before the first write of the new
#pragma unroll
    for (int u = 0; u < 6; u++)
        if (key[u] != KEY_NONE && rank[u] < kc)
        {
            buf[rank[u]] = key[u];
            if (rank[u] == kc - 1)
                *thr = key[u];
        }
    return c < kc ? c : kc;
}

/// grid: any size; slot -> work item (list, tile of TQ queries, row segment) as in sq_ivf_scan_kernel.  Dynamic LDS:
/// sqc_lds_bytes(TQ, ld, k).  TQ 32, or 16 where the records of 32 queries do not fit (the MFMA's other 16 columns idle).
/// A wavefront owns 32 rows of every group of 128: A = its rows' codes from global memory, 16 bytes a lane (row lane & 31, K half
/// lane >> 5), four K steps (128 bytes of a row) requested ahead of the MFMAs that use them; B = the queries' planes out of LDS.
/// acc[v] of lane (t, h) is row (v & 3) + 8 (v >> 2) + 4 h against query t: the lane scores 16 rows of ITS query, so the query's
/// terms and its threshold sit in the lane's registers.  Selection: keys below the query's threshold are appended to its LDS
/// buffer (one LDS atomic per lane and group); between groups the block meets, and a buffer that could overflow in the next group
/// (count > CAP - 128) is ranked by one wavefront and cut to its kc best, whose last becomes the threshold.  Nothing is sampled and
/// nothing is dropped but a key that kc better ones precede.  At the end every buffer is ranked and its kc best go out sorted.
template <int METRIC, int TQ>
__global__ __launch_bounds__(BLOCK) void sq_cand_scan_kernel(const SqCandParams a)
{
    const uint32_t ld = a.ld, kc = a.k, ld16 = ld >> 4, cap = sqc_cap(kc);
    const uint32_t rec = (uint32_t)sqc_record_bytes(ld);
    unsigned char * img = msvs_smem;                                         // [TQ][rec]
    uint64_t * buf = reinterpret_cast<uint64_t *>(msvs_smem + (size_t)TQ * rec); // [TQ][cap]
    uint64_t * thr = buf + (size_t)TQ * cap;                                 // [TQ]
    uint32_t * cnt = reinterpret_cast<uint32_t *>(thr + TQ);                 // [TQ]
    uint32_t * qpair = cnt + TQ;                                             // [TQ]
    float * qbase = reinterpret_cast<float *>(qpair + TQ);                   // [TQ] the pair's coarse term
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, i = lane & 31, t = i % TQ;
    const uint32_t nsteps = (ld16 + 1) >> 1, nchunks = (nsteps + 3) >> 2; // K steps of 32 bytes (the last may be half), chunks of four

    const uint32_t total = a.work_off[a.nlist];
    const uint32_t per_xcd = (total + 7) / 8;
    for (uint32_t s = blockIdx.x; s < 8 * per_xcd; s += gridDim.x)
    {
        const uint32_t w = ivf_slot_item(s, per_xcd);
        if (w >= total)
            continue;
        const IvfWorkItem it = ivf_work_item<TQ>(w, a.work_off, a.pair_off, a.list_off, a.nlist, a.rows_per_block);
        const uint32_t row_begin = it.row_begin, row_end = it.row_end;
        const uint32_t nvalid = min((uint32_t)TQ, it.pair_end - it.pair_begin);
        __syncthreads(); // the previous item is done with the LDS
        if (tid < nvalid)
        {
            const uint32_t qp = a.pairs[it.pair_begin + tid];
            qpair[tid] = qp;
            qbase[tid] = a.probe_dis[qp];
            cnt[tid] = 0;
            thr[tid] = KEY_NONE;
        }
        __syncthreads();
        for (uint32_t c = tid; c < nvalid * (rec >> 4); c += BLOCK) // the tile's records, verbatim
        {
            const uint32_t tq = c / (rec >> 4), off = c - tq * (rec >> 4);
            reinterpret_cast<uint4 *>(img)[c] = reinterpret_cast<const uint4 *>(a.img + (size_t)(qpair[tq] / a.nprobe) * rec)[off];
        }
        __syncthreads();
        const bool tvalid = i < nvalid; // (i >= TQ: the idle half of a 16-query tile)
        float qo = 0.f, delta = 0.f, base = 0.f;
        if (tvalid)
        {
            const float * tailf = reinterpret_cast<const float *>(img + (size_t)t * rec + 2 * ld);
            qo = tailf[0];
            delta = tailf[1];
            base = METRIC == M_IP ? __fadd_rn(qbase[t], qo) : qbase[t];
        }
        const unsigned char * bq = img + (size_t)t * rec + 16 * h; // the lane's B fragments: + 32 s (h plane), + ld + 32 s (l plane)

        for (uint32_t g0 = row_begin; g0 < row_end; g0 += SQC_GROUP)
        {
            const uint32_t r0 = g0 + 32 * wave;
            if (r0 < row_end) // (uniform over the wavefront)
            {
                const uint4 * arow = a.codes + (size_t)min(r0 + i, row_end - 1) * ld16 + h;
                auto load_chunk = [&](uint32_t c, uint4 * dst) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                    {
                        const uint32_t w16 = 2 * (4 * c + u) + h; // the lane's 16-byte word of the row
                        dst[u] = w16 < ld16 ? arow[2 * (4 * c + u)] : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
                    }
                };
                sqc_i32x16 ach = {}, acl = {};
                uint4 cur[4], nxt[4];
                load_chunk(0, nxt);
                for (uint32_t c = 0; c < nchunks; c++)
                {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        cur[u] = nxt[u];
                    if (c + 1 < nchunks)
                        load_chunk(c + 1, nxt);
#pragma unroll
                    for (int u = 0; u < 4; u++)
                    {
                        const uint32_t st = 4 * c + u;
                        if (st < nsteps) // (uniform)
                        {
                            // s = code - 128 as int8: one XOR per four codes (beyond the row: 0x80 ^ 0x80 = 0)
                            const sqc_i32x4 af = {(int)(cur[u].x ^ 0x80808080u), (int)(cur[u].y ^ 0x80808080u), (int)(cur[u].z ^ 0x80808080u),
                                                  (int)(cur[u].w ^ 0x80808080u)};
                            const sqc_i32x4 bh = *reinterpret_cast<const sqc_i32x4 *>(bq + 32 * st);
                            const sqc_i32x4 bl = *reinterpret_cast<const sqc_i32x4 *>(bq + ld + 32 * st);
                            ach = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bh, ach, 0, 0, 0);
                            acl = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bl, acl, 0, 0, 0);
                        }
                    }
                }
                // the rows' side: lane i looks at row r0 + i (both halves of the wavefront alike)
                const uint32_t r = r0 + i;
                bool rok = r < row_end;
                float er = 0.f;
                if (rok)
                {
                    if (METRIC == M_L2)
                        er = a.erow[r];
                    if (a.alive)
                    {
                        const uint32_t id = a.labels[r];
                        rok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
                    }
                }
                const uint32_t okmask = (uint32_t)__ballot(rok);
                const uint64_t floor_key = tvalid ? thr[t] : 0;
                uint64_t key[16];
                uint32_t n_new = 0;
#pragma unroll
                for (int v = 0; v < 16; v++)
                {
                    const uint32_t m = (v & 3) + 8 * (v >> 2) + 4 * h;
                    const float em = __shfl(er, (int)m);
                    const int64_t S = 128 * (int64_t)ach[v] + (int64_t)acl[v];
                    const float x = __fmul_rn(delta, (float)S);
                    float sc;
                    if (METRIC == M_IP)
                        sc = __fadd_rn(base, x);
                    else
                        sc = __fsub_rn(__fadd_rn(base, em), __fmul_rn(2.f, __fadd_rn(qo, x)));
                    const uint64_t kv = sqc_key<METRIC>(sc, r0 + m);
                    key[v] = ((okmask >> m) & 1) && kv < floor_key ? kv : KEY_NONE;
                    n_new += key[v] != KEY_NONE ? 1u : 0u;
                }
                if (n_new)
                {
                    uint32_t slot = atomicAdd(&cnt[t], n_new);
                    uint64_t * dst = buf + (size_t)t * cap;
#pragma unroll
                    for (int v = 0; v < 16; v++)
                        if (key[v] != KEY_NONE)
                            dst[slot++] = key[v];
                }
            }
            __syncthreads();
            for (uint32_t tq = wave; tq < nvalid; tq += 4) // (uniform) a buffer the next group could overflow is cut to its kc best
            {
                const uint32_t c = cnt[tq];
                if (c + SQC_GROUP > cap)
                {
                    const uint32_t kept = sqc_compact(buf + (size_t)tq * cap, c, kc, &thr[tq], lane);
                    if (lane == 0)
                        cnt[tq] = kept;
                }
            }
            __syncthreads();
        }
        for (uint32_t tq = wave; tq < nvalid; tq += 4) // the item's kc best of every query, sorted, KEY_NONE behind them
        {
            uint64_t * b = buf + (size_t)tq * cap;
            const uint32_t kept = sqc_compact(b, cnt[tq], kc, &thr[tq], lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint64_t * out = a.partial + ((size_t)qpair[tq] * a.seg_max + it.seg) * kc;
            for (uint32_t e = lane; e < kc; e += WAVE)
                out[e] = e < kept ? b[e] : KEY_NONE;
        }
    }
}

// ------------------------------------------------------------------------------------------ the re-rank

struct SqRerankParams
{
    const uint64_t * cand;   // [query of the round][kc] keys (a, position), KEY_NONE-padded
    const uint4 * codes;
    const uint32_t * labels;
    const float4 * Q;        // the round's queries, ld4 float4 each
    const float4 * cent, * vmin, * step;
    const int64_t * list_off;
    uint32_t nlist, ld4, kc, k;
    int cosine;
    int64_t * out_ids;       // [query of the round][k]
    float * out_dis;
};

/// A block per query, sixteen 16-lane groups: candidate i's row is decoded and scored exactly as sq_ivf_scan_kernel scores it (the
/// same columns per lane in the same order, the same fold, make_key's admission), then the kc keys (distance, label) are ranked
/// and the first k written; -1 / the metric's neutral value (cosine: fl(1 - it)) behind them, as the list scan's merge writes them.
template <int METRIC>
__global__ __launch_bounds__(BLOCK) void sq_cand_rerank_kernel(const SqRerankParams a)
{
    __shared__ uint64_t keys[MSVS_MAX_K];
    const uint32_t tid = threadIdx.x, g = tid & 15, q = blockIdx.x, ld4 = a.ld4;
    const float4 * qs = a.Q + (size_t)q * ld4;
    for (uint32_t c = tid >> 4; c < a.kc; c += 16)
    {
        const uint64_t ck = a.cand[(size_t)q * a.kc + c];
        uint64_t key = KEY_NONE;
        if (ck != KEY_NONE) // (uniform over the group)
        {
            const uint32_t pos = (uint32_t)ck;
            const float4 * cl = a.cent + (size_t)sqc_list_of(a.list_off, a.nlist, pos) * ld4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            sqc_for_columns(a.codes + (size_t)pos * (ld4 >> 2), ld4, g, [&](uint32_t col, uint32_t w) {
                const float4 e = sqc_inner(w, a.vmin[col], a.step[col]), cc = cl[col], qq = qs[col];
                const float4 y = make_float4(__fadd_rn(cc.x, e.x), __fadd_rn(cc.y, e.y), __fadd_rn(cc.z, e.z), __fadd_rn(cc.w, e.w));
                if (METRIC == M_L2)
                {
                    const float4 dlt = make_float4(__fsub_rn(qq.x, y.x), __fsub_rn(qq.y, y.y), __fsub_rn(qq.z, y.z), __fsub_rn(qq.w, y.w));
                    sqc_mac(acc, dlt, dlt);
                }
                else
                    sqc_mac(acc, qq, y);
            });
            key = make_key<METRIC>(sqc_fold(acc), a.labels[pos]);
        }
        if (g == 0)
            keys[c] = key;
    }
    __syncthreads();
    if (tid < a.kc)
    {
        const uint64_t key = keys[tid];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < a.kc; j++)
            rank += keys[j] < key || (keys[j] == key && j < tid) ? 1u : 0u;
        if (rank < a.k)
        {
            const size_t o = (size_t)q * a.k + rank;
            a.out_ids[o] = key == KEY_NONE ? -1 : (int64_t)(uint32_t)key;
            const float v = key_value<METRIC>(key);
            a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
        }
    }
}

}
