// refine_kernels.hpp -- the second stage of a two-stage search (refine.hip): the candidate labels of every query are
// scored against the f32 rows of a row store (row i is label i) with the canonical scan arithmetic, ranked, and the best k written.
//
// One block of 256 threads per query.  The query sits in LDS once (ld4 x 16 bytes); sixteen 16-lane groups take the candidates
// grp, grp + 16, ...; a lane owns the float4 pieces g, g + 16, ... of the row and walks them with canonical_row_chain (whole batches
// of twelve requests in flight), the 64 partial sums fold through row16_tree_sum, make_key turns the value into the ordered key
// (strict admission, NaN never) and the key goes to LDS slot c of kc (<= 8 KiB).  A group's request is 256 contiguous bytes of one
// row, which is what keeps the gather tolerable when the table is mapped host memory: the kernel does not know the placement.
// Every key then ranks itself among the kc slots -- (key, slot) ascending, so a label that occurs twice gets two ranks -- and the
// ranks below k are written; padding labels (< 0, >= num) are KEY_NONE and rank behind every admitted key.
#pragma once

#include "mfma_scan_kernels.hpp"
#include "scan_kernels.hpp"

#pragma clang fp contract(off)

namespace msvs
{

struct RefineParams
{
    const float4 * rows;  // num x ld4, zero padded; HBM or mapped pinned host memory
    const float4 * Q;     // nq x ld4, zero padded (normalised for cosine)
    const int64_t * cand; // nq x kc labels
    int64_t * out_ids;    // nq x k
    float * out_dis;      // nq x k
    uint64_t num;         // rows in the store: labels outside [0, num) are skipped
    uint32_t ld4, kc, k;
    int cosine; // report fl(1 - ip) in every slot
};

inline size_t refine_lds_bytes(uint32_t ld4, uint32_t kc) { return (size_t)ld4 * 16 + (size_t)kc * 8; }

/// U keys per thread (slots tid, tid + 256, ...) rank themselves among keys[0 .. kc) in one pass over the slots; ranks below k go out
template <int METRIC, int U>
__device__ __forceinline__ void refine_rank_write(const RefineParams & a, const uint64_t * keys, const uint32_t q, const uint32_t tid)
{
    uint64_t mine[U];
    uint32_t rank[U];
#pragma unroll
    for (int u = 0; u < U; u++)
    {
        const uint32_t i = tid + u * BLOCK;
        mine[u] = i < a.kc ? keys[i] : KEY_NONE;
        rank[u] = 0;
    }
    for (uint32_t j = 0; j < a.kc; j++)
    {
        const uint64_t kj = keys[j]; // one address for the whole block: a broadcast read
#pragma unroll
        for (int u = 0; u < U; u++)
            rank[u] += kj < mine[u] || (kj == mine[u] && j < tid + u * BLOCK) ? 1u : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if (tid + u * BLOCK < a.kc && rank[u] < a.k)
        {
            const size_t o = (size_t)q * a.k + rank[u];
            a.out_ids[o] = mine[u] == KEY_NONE ? -1 : (int64_t)(uint32_t)mine[u];
            const float v = key_value<METRIC>(mine[u]);
            a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
        }
}

template <int METRIC>
static __global__ __launch_bounds__(BLOCK) void refine_kernel(const RefineParams a)
{
    extern __shared__ __align__(16) unsigned char refine_lds[];
    float4 * qs = reinterpret_cast<float4 *>(refine_lds);
    uint64_t * keys = reinterpret_cast<uint64_t *>(refine_lds + (size_t)a.ld4 * 16);
    const uint32_t q = blockIdx.x, tid = threadIdx.x, grp = tid >> 4, g = tid & 15;
    const uint32_t ld4 = a.ld4, kc = a.kc;
    for (uint32_t i = tid; i < ld4; i += BLOCK)
        qs[i] = a.Q[(size_t)q * ld4 + i];
    __syncthreads();
    const uint32_t jfull = ld4 >> 4, jtail = ld4 & 15;
    const float4 * qrow = qs + g;
    for (uint32_t c = grp; c < kc; c += 16)
    {
        const int64_t label = a.cand[(size_t)q * kc + c]; // uniform over the 16 lanes that own candidate c
        if (label < 0 || (uint64_t)label >= a.num)
        {
            if (g == 0)
                keys[c] = KEY_NONE;
            continue;
        }
        uint32_t id = (uint32_t)label;
        const float4 acc = canonical_row_chain<METRIC>(a.rows + (size_t)label * ld4 + g, qrow, jfull, jtail, g, nullptr, id);
        float s = __fadd_rn(__fadd_rn(acc.x, acc.y), __fadd_rn(acc.z, acc.w));
        s = row16_tree_sum(s);
        if (g == 0)
            keys[c] = make_key<METRIC>(s, id);
    }
    __syncthreads();
    if (kc <= BLOCK)
        refine_rank_write<METRIC, 1>(a, keys, q, tid);
    else
        refine_rank_write<METRIC, 4>(a, keys, q, tid); // kc <= MSVS_REFINE_MAX_CAND = 4 * BLOCK
    // k may exceed kc: the rest are pads
    for (uint32_t i = kc + tid; i < a.k; i += BLOCK)
    {
        const size_t o = (size_t)q * a.k + i;
        a.out_ids[o] = -1;
        const float v = key_value<METRIC>(KEY_NONE);
        a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
    }
}

}
