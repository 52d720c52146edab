// sq_ivf_kernels.hpp -- device code of the IVFSQ index (sq_index.hip): 8-bit residual codes are ALL the index keeps of a row.
//
//   quantiser : one per index, vmin[j] / step[j] per dimension, step = fl(fl(vmax - vmin) / 255);
//   encode    : r = fl(x - c_l), t = fl(fl(r - vmin) / step), code = min(255, max(0, rint(t))), 0 where step == 0;
//   decode    : x^ = fl(c_l + fl(vmin + fl(float(code) * step)));
//   search    : the canonical arithmetic of scan_rows (scan_kernels.hpp) over the DECODED rows -- a 16-lane group owns a row, lane g
//               owns float4 columns g, g + 16, ...; only the origin of the row operand differs (decoded in registers instead of
//               loaded), so ids and distances are those of oracle.ivf_search over the decoded matrix, bit for bit.
//
// Stored row: ldc = round_up(dim, 16) bytes.  Inside every whole block of 256 columns the bytes are permuted so that the 16 bytes at
// offset 256 b + 16 g are the four float4 columns 64 b + g, + 16, + 32, + 48 of lane g (one 16-byte load = four of the lane's own
// columns, in its accumulation order); the tail (ldc mod 256 bytes) stays in natural order and a lane reads one 32-bit word per
// column there.  sq_stored_pos is the map, used by the encoder and undone by the export.
//
// Two more code widths (BITS, create's bit_size) share every kernel here; only the origin of the decoded column differs:
//   BITS  4 : the quantiser above with 15 in place of 255; two codes a stored byte, 32 codes = eight of the lane's columns per load;
//   BITS 16 : code = the binary16 nearest to r (ties to even, subnormals kept, overflow to +-inf), x^ = fl(c_l + float(code));
//             vmin / step are not read; 8 halves = two of the lane's columns per load.
// Their stored orders and maps: sq_layout.hpp.
#pragma once

#include "scan_kernels.hpp"
#include "sq_layout.hpp"

namespace msvs
{

// ------------------------------------------------------------------------------------------ range of the training residuals

/// omin[j] / omax[j] = min / max over the rows of f2ord(fl(x_j - c_lj)) (ordered-float atomics; omin starts at 0xFFFFFFFF, omax at 0).
/// A block takes `rows_per_block` rows, thread t the columns t, t + 256, ...: one pair of atomics per (block, column).
static __global__ __launch_bounds__(BLOCK) void sq_range_kernel(const float * X, const int32_t * list, const float * C, size_t n, uint32_t d,
                                                                uint32_t ld, uint32_t rows_per_block, uint32_t * omin, uint32_t * omax)
{
    const size_t r0 = (size_t)blockIdx.x * rows_per_block;
    const size_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    for (uint32_t j = threadIdx.x; j < d; j += BLOCK)
    {
        uint32_t lo = 0xFFFFFFFFu, hi = 0;
        for (size_t r = r0; r < r1; r++)
        {
            const float v = __fsub_rn(X[r * ld + j], C[(size_t)list[r] * ld + j]);
            if (v == v) // (a NaN has no place in a range)
            {
                const uint32_t o = f2ord(v);
                lo = o < lo ? o : lo;
                hi = o > hi ? o : hi;
            }
        }
        if (lo <= hi)
        {
            atomicMin(&omin[j], lo);
            atomicMax(&omax[j], hi);
        }
    }
}

// ------------------------------------------------------------------------------------------ encode

/// the code (0 .. top) of column j < d of row r against the centroid of list[r]
__device__ inline float sq_code(const float * X, const int32_t * list, const float * C, const float * vmin, const float * step, size_t r,
                                uint32_t j, uint32_t ld, float top)
{
    const float st = step[j];
    if (st == 0.f)
        return 0.f;
    const float res = __fsub_rn(X[r * ld + j], C[(size_t)list[r] * ld + j]);
    const float t = __fdiv_rn(__fsub_rn(res, vmin[j]), st);
    return fminf(top, fmaxf(0.f, rintf(t))); // rintf: to nearest, ties to even
}

/// BITS 8: codes[r][sq_stored_pos(j)] = code of column j of row r against the centroid of list[r]; columns d .. ldc - 1 are 0.
/// One thread per (row, natural column).
/// BITS 16: the same with halves: the binary16 bits of the residual at half sq16_stored_pos(j) (vmin, step: not read).
/// BITS 4: one thread per (row, STORED byte), which holds the codes of two natural columns (sq4_stored_cols): no two threads
/// write one byte; pad nibbles and pad columns are 0.
/// ldc: elements of a row the grid covers = ld (BITS 8, 16) or the row's bytes (BITS 4).
template <int BITS>
__global__ __launch_bounds__(BLOCK) void sq_encode_kernel(const float * X, const int32_t * list, const float * C, const float * vmin,
                                                          const float * step, size_t n, uint32_t d, uint32_t ld, uint32_t ldc, uint8_t * codes)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n * ldc)
        return;
    const size_t r = i / ldc;
    const uint32_t j = (uint32_t)(i - r * ldc);
    if (BITS == 8)
    {
        const float code = j < d ? sq_code(X, list, C, vmin, step, r, j, ld, 255.f) : 0.f;
        codes[r * ldc + sq_stored_pos(j, ldc)] = (uint8_t)code;
    }
    else if (BITS == 4)
    {
        uint32_t jl, jh;
        sq4_stored_cols(j, ld, jl, jh);
        const float lo = jl < d ? sq_code(X, list, C, vmin, step, r, jl, ld, 15.f) : 0.f;
        const float hi = jh < d ? sq_code(X, list, C, vmin, step, r, jh, ld, 15.f) : 0.f;
        codes[r * ldc + j] = (uint8_t)((uint32_t)lo | ((uint32_t)hi << 4));
    }
    else
    {
        _Float16 h = (_Float16)0.f;
        if (j < d)
            h = (_Float16)__fsub_rn(X[r * ld + j], C[(size_t)list[r] * ld + j]); // to nearest even, subnormals kept, overflow to +-inf
        reinterpret_cast<_Float16 *>(codes)[r * ldc + sq16_stored_pos(j, ldc)] = h;
    }
}

/// dst[pos[i]] = src[i] for rows of ld16 16-byte words (the staged chunks into their list-major places)
static __global__ void sq_scatter_rows_kernel(const uint4 * src, uint4 * dst, const uint32_t * pos, size_t n, uint32_t ld16)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * ld16)
        return;
    const size_t r = i / ld16;
    dst[(size_t)pos[r] * ld16 + (i - r * ld16)] = src[i];
}

// ------------------------------------------------------------------------------------------ list scan

struct SqIvfParams
{
    const uint4 * codes;     // rows, list-major, sq_row_words(BITS, 4 ld4) uint4 each (stored order)
    const uint32_t * labels; // label of row r
    const uint64_t * alive;  // nullable filter bitmap over labels
    const float4 * Q;        // queries, ld4 float4 each (zero padded)
    const float4 * cent;     // [nlist][ld4]
    const float4 * vmin, * step; // [ld4], zero padded (BITS 16: not read)
    uint64_t * partial;      // [(pair * seg_max + segment)][k]
    uint32_t nbits, ld4, k;
    uint32_t nprobe;         // probes per query (pair i = q * nprobe + p)
    uint32_t nlist, rows_per_block, seg_max;
    const int64_t * list_off; // [nlist + 1]
    const uint32_t * pair_off, * work_off, * pairs; // the plan (IvfPlanParams)
    const uint64_t * after;  // AFTER 1 only: [query of the round] continuation keys (search in rounds, coded_ivf.hpp)
};

/// LDS bytes of a scan block: the tile's queries, the list's centroid, vmin and step (not at 16 bits), and the merge lists.
inline size_t sq_lds_bytes(uint32_t T, uint32_t ld4, uint32_t k, uint32_t bits = 8)
{
    return (size_t)(T + (bits == 16 ? 1 : 3)) * ld4 * 16 + (size_t)T * 5 * k * 8;
}

/// grid: any size; slot -> work item (list, query tile, row segment) as in ivf_batched_scan_kernel (an XCD walks one contiguous range).
/// dynamic LDS: sq_lds_bytes(T, ld4, k, BITS).
/// BITS: the code width.  A unit is E = 128 / (4 BITS) float4 columns per lane (16 E per group): one 16-byte load inside a whole
/// block, narrower loads of the same columns in the natural-order tail; the lane's columns come out of it in ascending order.
/// AFTER 1 (a later round of a search with k > MSVS_MAX_K): a row is offered to tile query t only if its key is strictly greater
/// than a.after[query of t], the last key the query has returned; KEY_NONE there admits nothing.  The floor is read once per work
/// item and is uniform over the workgroup (scalar registers).  AFTER 0 never reads a.after.
template <int BITS, int METRIC, int T, int R, int AFTER = 0>
__global__ __launch_bounds__(BLOCK) void sq_ivf_scan_kernel(const SqIvfParams a)
{
    static_assert(BITS == 4 || BITS == 8 || BITS == 16, "code widths of the IVFSQ index");
    constexpr uint32_t E = 32 / BITS; // float4 columns of a lane per unit
    const uint32_t ld4 = a.ld4, k = a.k;
    float4 * qs = reinterpret_cast<float4 *>(msvs_smem);     // [T][ld4]
    float4 * cs = qs + (size_t)T * ld4;                      // [ld4] centroid of the item's list
    float4 * vm = cs + ld4;                                  // [ld4] (BITS 16: neither vm nor st is there)
    float4 * st = vm + ld4;                                  // [ld4]
    uint64_t * lds_merge = reinterpret_cast<uint64_t *>(BITS == 16 ? vm : st + ld4);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4, g = lane & 15;
    const uint32_t ld16 = BITS == 8 ? ld4 >> 2 : sq_row_words(BITS, ld4 << 2); // 16-byte words per stored row
    const uint32_t nb = ld4 / (16 * E);   // whole blocks of 256 stored bytes (64 E columns)
    const uint32_t nu = nb + ((ld4 & (16 * E - 1)) ? 1 : 0); // units per row: the blocks, then the tail
    if (BITS != 16)
        for (uint32_t c = tid; c < ld4; c += BLOCK)
        {
            vm[c] = a.vmin[c];
            st[c] = a.step[c];
        }

    auto fma4 = [&](float4 & s, const float4 q, const float4 y) {
        if (METRIC == M_L2)
        {
            float dx = __fsub_rn(q.x, y.x), dy = __fsub_rn(q.y, y.y), dz = __fsub_rn(q.z, y.z), dw = __fsub_rn(q.w, y.w);
            s.x = __fadd_rn(s.x, __fmul_rn(dx, dx));
            s.y = __fadd_rn(s.y, __fmul_rn(dy, dy));
            s.z = __fadd_rn(s.z, __fmul_rn(dz, dz));
            s.w = __fadd_rn(s.w, __fmul_rn(dw, dw));
        }
        else
        {
            s.x = __fadd_rn(s.x, __fmul_rn(q.x, y.x));
            s.y = __fadd_rn(s.y, __fmul_rn(q.y, y.y));
            s.z = __fadd_rn(s.z, __fmul_rn(q.z, y.z));
            s.w = __fadd_rn(s.w, __fmul_rn(q.w, y.w));
        }
    };
    // four codes (one float4 column) -> the decoded column
    auto decode4 = [&](uint32_t w, uint32_t col) {
        const float4 c = cs[col], m = vm[col], s = st[col];
        float4 y;
        y.x = __fadd_rn(c.x, __fadd_rn(m.x, __fmul_rn((float)(w & 255u), s.x)));
        y.y = __fadd_rn(c.y, __fadd_rn(m.y, __fmul_rn((float)((w >> 8) & 255u), s.y)));
        y.z = __fadd_rn(c.z, __fadd_rn(m.z, __fmul_rn((float)((w >> 16) & 255u), s.z)));
        y.w = __fadd_rn(c.w, __fadd_rn(m.w, __fmul_rn((float)(w >> 24), s.w)));
        return y;
    };
    // four halves (one float4 column) -> the decoded column
    auto decode4h = [&](uint32_t w0, uint32_t w1, uint32_t col) {
        typedef _Float16 half2v __attribute__((ext_vector_type(2)));
        const half2v lo = __builtin_bit_cast(half2v, w0), hi = __builtin_bit_cast(half2v, w1);
        const float4 c = cs[col];
        float4 y;
        y.x = __fadd_rn(c.x, (float)lo[0]);
        y.y = __fadd_rn(c.y, (float)lo[1]);
        y.z = __fadd_rn(c.z, (float)hi[0]);
        y.w = __fadd_rn(c.w, (float)hi[1]);
        return y;
    };
    // BITS 4, the natural-order tail: four nibbles -> a word of four byte-codes
    auto spread4 = [](uint32_t h) { return (h & 0xfu) | ((h & 0xf0u) << 4) | ((h & 0xf00u) << 8) | ((h & 0xf000u) << 12); };

    const uint32_t total = a.work_off[a.nlist];
    const uint32_t per_xcd = (total + 7) / 8;
    for (uint32_t s = blockIdx.x; s < 8 * per_xcd; s += gridDim.x)
    {
        const uint32_t w = ivf_slot_item(s, per_xcd);
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
            const float4 * src = a.Q + (size_t)(qp / a.nprobe) * ld4;
            for (uint32_t c = tid; c < ld4; c += BLOCK)
                qs[t * ld4 + c] = src[c];
        }
        for (uint32_t c = tid; c < ld4; c += BLOCK)
            cs[c] = a.cent[(size_t)l * ld4 + c];
        __syncthreads();

        WaveTopK<R> top[T];
#pragma unroll
        for (int t = 0; t < T; t++)
            top[t].init();

        // unit u of the row of this lane's group at step `base`: a whole block -> the lane's 16 bytes of it; the tail -> one 32-bit word
        // (BITS 16: 64 bits, BITS 4: 16 bits) per column the lane owns there (0 beyond the row), in the block's order of columns
        auto load_unit = [&](uint32_t base, uint32_t u) {
            const uint32_t r = min(base + grp, row_end - 1);
            const uint4 * row = a.codes + (size_t)r * ld16;
            if (u < nb)
                return row[u * 16 + g];
            const uint32_t tc = ld4 & (16 * E - 1);
            uint4 v;
            if (BITS == 8)
            {
                const uint32_t * tail = reinterpret_cast<const uint32_t *>(row) + nb * 64;
                v.x = g < tc ? tail[g] : 0u;
                v.y = g + 16 < tc ? tail[g + 16] : 0u;
                v.z = g + 32 < tc ? tail[g + 32] : 0u;
                v.w = g + 48 < tc ? tail[g + 48] : 0u;
            }
            else if (BITS == 16)
            {
                const uint2 * tail = reinterpret_cast<const uint2 *>(row) + nb * 32;
                const uint2 c0 = g < tc ? tail[g] : make_uint2(0u, 0u), c1 = g + 16 < tc ? tail[g + 16] : make_uint2(0u, 0u);
                v = make_uint4(c0.x, c0.y, c1.x, c1.y);
            }
            else
            {
                const uint16_t * tail = reinterpret_cast<const uint16_t *>(row) + nb * 128;
                uint32_t h[8];
#pragma unroll
                for (int e = 0; e < 8; e++)
                    h[e] = g + 16 * e < tc ? (uint32_t)tail[g + 16 * e] : 0u;
                v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
            return v;
        };

        uint32_t base = row_begin + wave * 4;
        uint4 wnext = make_uint4(0, 0, 0, 0);
        if (base < row_end)
            wnext = load_unit(base, 0);
        for (; base < row_end; base += 16)
        {
            const uint32_t r = base + grp;
            const bool rv = r < row_end;
            float4 acc[T];
#pragma unroll
            for (int t = 0; t < T; t++)
                acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (uint32_t u = 0; u < nu; u++)
            {
                const uint4 cw = wnext;
                // the next unit's codes are on their way while this one is decoded: the row's next unit, or the next step's first
                if (u + 1 < nu)
                    wnext = load_unit(base, u + 1);
                else if (base + 16 < row_end)
                    wnext = load_unit(base + 16, 0);
                const uint32_t col0 = u * (16 * E) + g; // the lane's columns of this unit: col0, + 16, ... (E of them, ascending)
                const uint32_t words[4] = {cw.x, cw.y, cw.z, cw.w};
                uint32_t planes[BITS == 4 ? 8 : 1]; // BITS 4: a word of four byte-codes per column
                if constexpr (BITS == 4)
                {
                    if (u < nb) // (uniform) a block keeps two columns a word as nibble planes, the tail as 16-bit halves
                    {
#pragma unroll
                        for (int e = 0; e < 8; e++)
                            planes[e] = ((e & 1) ? words[e >> 1] >> 4 : words[e >> 1]) & 0x0f0f0f0fu;
                    }
                    else
                    {
#pragma unroll
                        for (int e = 0; e < 8; e++)
                            planes[e] = spread4((e & 1) ? words[e >> 1] >> 16 : words[e >> 1] & 0xffffu);
                    }
                }
#pragma unroll
                for (int e = 0; e < (int)E; e++)
                {
                    const uint32_t col = col0 + 16 * e;
                    if (col < ld4)
                    {
                        float4 y;
                        if constexpr (BITS == 8)
                            y = decode4(words[e], col);
                        else if constexpr (BITS == 16)
                            y = decode4h(words[2 * e], words[2 * e + 1], col);
                        else
                            y = decode4(planes[e], col);
#pragma unroll
                        for (int t = 0; t < T; t++)
                            fma4(acc[t], qs[t * ld4 + col], y);
                    }
                }
            }
            // id + filter of the finished row (lane g == 0 of its group offers it), the cross-lane sum in tree order, the offers
            uint32_t id = 0;
            bool ok = rv && g == 0;
            if (ok)
            {
                id = a.labels[r];
                if (a.alive)
                    ok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
            }
#pragma unroll
            for (int t = 0; t < T; t++)
            {
                float sum = __fadd_rn(__fadd_rn(acc[t].x, acc[t].y), __fadd_rn(acc[t].z, acc[t].w));
                sum = row16_tree_sum(sum);
                uint64_t key = ok ? make_key<METRIC>(sum, id) : KEY_NONE;
                if (AFTER)
                    key = key > floor_key[t] ? key : KEY_NONE;
                top[t].offer(key, k, lane);
            }
        }

        tile_rank_merge<T, R>(top, lds_merge, out, k); // (no barrier in front: the row loop reads the staged rows and tables, not lds_merge)
    }
}

}
