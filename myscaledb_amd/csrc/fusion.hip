// fusion.hip -- msvs_hybrid_fuse_device (include/msvs.h): the fusion step of a hybrid search for a BATCH of queries on the
// device, straight from the two device searches' output arrays.
//
// Follows RankFusion / RelativeScoreFusion / computeNormalizedScore (src/VectorIndex/Utils/HybridSearchUtils.cpp:164-300) as
// MergeTreeHybridSearchManager::hybridSearch applies them -- the arithmetic and order of msvs_host_hybrid_search_batch
// (host/msvs_host.cpp), which tests hold against the map-based mirror: a label's contributions are applied in list order
// (RRF: 0 + 1/(k + rank_vector), then + 1/(k + rank_text); RSF: the text list ASSIGNS weight * norm, the vector list adds),
// output = descending fused score, ties by ascending label; a NaN fused score (RSF: a +inf distance at the head of a finite list
// normalises to inf / inf) ranks behind every other score, NaN scores among themselves by ascending label.
// A hybrid batch of 64 queries spent 0.6 of its 2.7 ms in that host loop behind a stream synchronisation and four
// device-to-host copies; here the lists never leave the device and only the top-k rows are read back.
//
// One workgroup per query, thread i = entry i of (vector list | text list), both <= 256 long.  Every entry looks its label
// up in the other list (LDS, <= 256 compares); an entry is the OWNER of its label when it is the vector entry, or a text
// entry without a vector partner; owners rank themselves against each other by (score desc, label asc) and write themselves
// to their output slot.  The lists hold distinct labels each (row ids of one search: the precondition of include/msvs.h; with a
// repeated label two owners can share a rank or a hash chain a partner, and every access stays in bounds).
//
// Longer lists (up to FUSE_LONG_MAX = MSVS_MAX_K_ROUNDS rows each: a hybrid search asks both sides for 3 x LIMIT candidates) take
// hybrid_fuse_long_kernel: the same arithmetic in the same order, but the all-pairs compares (4096 x 4096) give way to a hash table
// of the text labels for the partner and a bitonic sort of the owners for the ranks.
#include <algorithm>
#include <mutex>

#include "device_ops.hpp"

#pragma clang fp contract(off)

namespace msvs
{

constexpr uint32_t FUSE_MAX = 256; // entries per list (MSVS_MAX_K) of hybrid_fuse_kernel
constexpr uint32_t FUSE_LONG_MAX = MSVS_MAX_K_ROUNDS; // ... of hybrid_fuse_long_kernel
constexpr uint32_t FUSE_LONG_THREADS = 1024;
constexpr uint64_t FUSE_NO_LABEL = ~0ull; // (labels are row ids >= 0)

struct FuseParams
{
    const float * vec_dis;
    const int64_t * vec_ids;
    const float * txt_scores;
    const int64_t * txt_ids;
    uint32_t kv, kt, nq, topk;
    int rsf;
    uint64_t fusion_k;
    float weight;
    int direction;
    float * out_scores;
    int64_t * out_labels;
    uint32_t * n_out;
};

/// computeNormalizedScore: (score - min) / (max - min) with min / max = last / first entry (swapped when descending);
/// all equal: 1.
__device__ __forceinline__ float fuse_norm(const float s, const float first, const float last)
{
    float mn = last, mx = first;
    if (mn == mx)
        return 1.0f;
    if (mn > mx)
    {
        const float t = mn;
        mn = mx;
        mx = t;
    }
    return __fdiv_rn(__fsub_rn(s, mn), __fsub_rn(mx, mn));
}

/// The rank order of the output -- descending fused score, ties by ascending label, NaN scores behind every other score and by
/// ascending label among themselves -- compares integer keys, so that a NaN costs the ranking loops nothing.  fuse_key: a score as
/// an unsigned key that ascends with the score; 0 is left to the entries that do not rank (empty slots, non-owners), NaN is 1, every
/// other score the sign-flipped bit pattern (-inf, the least: 0x007FFFFF), which fuse_key_score turns back into the score (a NaN
/// comes back as the canonical one).  fuse_order_key: the key as the order compares it: -0.0 (0x7FFFFFFF) ties with +0.0.
constexpr uint32_t FUSE_KEY_NAN = 1u, FUSE_KEY_NEG_ZERO = 0x7FFFFFFFu;

__device__ __forceinline__ uint32_t fuse_key(const float s)
{
    if (s != s)
        return FUSE_KEY_NAN;
    const uint32_t b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float fuse_key_score(const uint32_t k)
{
    if (k == FUSE_KEY_NAN)
        return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ uint32_t fuse_order_key(const uint32_t k) { return k + (k == FUSE_KEY_NEG_ZERO ? 1u : 0u); }

static __global__ __launch_bounds__(2 * FUSE_MAX) void hybrid_fuse_kernel(const FuseParams p)
{
    __shared__ uint64_t s_label[2 * FUSE_MAX];
    __shared__ float s_value[2 * FUSE_MAX];
    __shared__ uint32_t s_key[2 * FUSE_MAX]; // fuse_order_key of the owners' fused scores (>= 1); non-owners: 0
    __shared__ uint32_t s_n[3]; // nv, nt, owners
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const int64_t * vi = p.vec_ids + (size_t)q * p.kv, * ti = p.txt_ids + (size_t)q * p.kt;
    const float * vs = p.vec_dis + (size_t)q * p.kv, * ts = p.txt_scores + (size_t)q * p.kt;
    if (tid < 3)
        s_n[tid] = 0;
    __syncthreads();
    // list lengths: the first id < 0 ends a list (the host's `> -1` unpack; ids after it are not read)
    if (tid == 0)
    {
        uint32_t nv = 0, nt = 0;
        while (nv < p.kv && vi[nv] > -1)
            nv++;
        while (nt < p.kt && ti[nt] > -1)
            nt++;
        s_n[0] = nv;
        s_n[1] = nt;
    }
    __syncthreads();
    const uint32_t nv = s_n[0], nt = s_n[1];
    const bool is_vec = tid < FUSE_MAX;
    const uint32_t i = is_vec ? tid : tid - FUSE_MAX;
    const bool have = is_vec ? i < nv : i < nt;
    uint64_t label = 0;
    float value = 0.f;
    if (have)
    {
        label = (uint64_t)(is_vec ? vi[i] : ti[i]);
        if (!p.rsf)
            value = __fdiv_rn(1.0f, (float)(p.fusion_k + (uint64_t)(i + 1)));
        else if (is_vec)
        {
            const float n = fuse_norm(vs[i], vs[0], vs[nv - 1]);
            const float w1 = __fsub_rn(1.0f, p.weight);
            value = p.direction == -1 ? __fmul_rn(n, w1) : __fmul_rn(__fsub_rn(1.0f, n), w1);
        }
        else
            value = __fmul_rn(fuse_norm(ts[i], ts[0], ts[nt - 1]), p.weight);
    }
    s_label[tid] = label;
    s_value[tid] = value;
    __syncthreads();
    // the partner in the other list
    bool owner = have;
    float score = 0.f;
    if (have)
    {
        const uint32_t ob = is_vec ? FUSE_MAX : 0, on = is_vec ? nt : nv;
        int partner = -1;
        for (uint32_t j = 0; j < on; j++)
            if (s_label[ob + j] == label)
            {
                partner = (int)j;
                break;
            }
        if (is_vec)
        {
            // RRF: (0 + vector) + text; RSF: text assigns, vector adds
            if (p.rsf)
                score = partner >= 0 ? __fadd_rn(s_value[ob + partner], value) : __fadd_rn(0.0f, value);
            else
                score = partner >= 0 ? __fadd_rn(__fadd_rn(0.0f, value), s_value[ob + partner]) : __fadd_rn(0.0f, value);
        }
        else
        {
            owner = partner < 0;
            score = p.rsf ? value : __fadd_rn(0.0f, value);
        }
    }
    const uint32_t key = owner ? fuse_order_key(fuse_key(score)) : 0u;
    s_key[tid] = key;
    __syncthreads();
    if (owner)
    {
        // the owners before this one: a greater key (a better score; NaN has the least key of the owners), or an equal one with a
        // smaller label; a non-owner's key 0 is neither
        uint32_t rank = 0;
        for (uint32_t j = 0; j < 2 * FUSE_MAX; j++)
        {
            const uint32_t kj = s_key[j];
            rank += (kj > key || (kj == key && s_label[j] < label)) ? 1u : 0u;
        }
        atomicAdd(&s_n[2], 1u);
        if (rank < p.topk)
        {
            p.out_scores[(size_t)q * p.topk + rank] = score;
            p.out_labels[(size_t)q * p.topk + rank] = (int64_t)label;
        }
    }
    __syncthreads();
    const uint32_t n = s_n[2] < p.topk ? s_n[2] : p.topk;
    if (tid == 0)
        p.n_out[q] = n;
    if (tid >= n && tid < p.topk)
    {
        p.out_scores[(size_t)q * p.topk + tid] = 0.f;
        p.out_labels[(size_t)q * p.topk + tid] = -1;
    }
}

/// The rank order over (label, fuse_key) entries: an empty slot (key 0, FUSE_NO_LABEL) sorts behind every entry, two of them are
/// equal.  A strict total order over distinct labels, NaN included (the bitonic network needs one).
__device__ __forceinline__ bool fuse_before(const uint64_t la, const uint32_t ka, const uint64_t lb, const uint32_t kb)
{
    const uint32_t a = fuse_order_key(ka), b = fuse_order_key(kb);
    return a > b || (a == b && la < lb);
}

/// Lists of up to FUSE_LONG_MAX rows: one workgroup per query, both lists in LDS (entry i of the vector list at i, of the text list at
/// P + i, P = the power of two at or above the longer list).
///   1. list lengths (the first id < 0 ends a list) by an LDS minimum; labels and per-list values as in hybrid_fuse_kernel;
///   2. the text labels go into an open-addressing hash table (2 P slots: at most half full); every vector entry looks its label up,
///      adds its partner's value in the prescribed order and takes the partner out of the ranking;
///   3. the owners (label, fuse_key of the fused score) are sorted in place by fuse_before (bitonic, 2 P entries); the first topk leave.
/// Dynamic LDS sized by P (fuse_long_lds_bytes: 33 P bytes -- 16.5 KB for the 300-row lists of a LIMIT 100 hybrid search, 132 of the
/// 160 KB at 4096 rows) and min(P, 1024) threads, so that short lists share a CU.
inline size_t fuse_long_lds_bytes(uint32_t P) { return (size_t)P * (2 * 8 + 2 * 4 + 2 * 4 + 1); }

static __global__ __launch_bounds__(FUSE_LONG_THREADS) void hybrid_fuse_long_kernel(const FuseParams p, const uint32_t P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fuse_smem[];
    uint64_t * const s_label = reinterpret_cast<uint64_t *>(fuse_smem);       // [2 P]
    uint32_t * const s_bits = reinterpret_cast<uint32_t *>(s_label + 2 * P);  // [2 P] a value's float bits; from the fused scores on: fuse_key
    uint32_t * const s_tab = s_bits + 2 * P;                                    // [2 P] text entry + 1 (0: empty)
    uint8_t * const s_taken = reinterpret_cast<uint8_t *>(s_tab + 2 * P);     // [P] text entry has a vector partner
    __shared__ uint32_t s_n[3];                                               // nv, nt, owners
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int64_t * vi = p.vec_ids + (size_t)q * p.kv, * ti = p.txt_ids + (size_t)q * p.kt;
    const float * vs = p.vec_dis + (size_t)q * p.kv, * ts = p.txt_scores + (size_t)q * p.kt;
    const uint32_t N = 2 * P, tmask = N - 1;
    if (tid == 0)
    {
        s_n[0] = p.kv;
        s_n[1] = p.kt;
        s_n[2] = 0;
    }
    for (uint32_t i = tid; i < N; i += nthreads)
        s_tab[i] = 0;
    for (uint32_t i = tid; i < P; i += nthreads)
        s_taken[i] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < P; i += nthreads)
    {
        if (i < p.kv && !(vi[i] > -1))
            atomicMin(&s_n[0], i);
        if (i < p.kt && !(ti[i] > -1))
            atomicMin(&s_n[1], i);
    }
    __syncthreads();
    const uint32_t nv = s_n[0], nt = s_n[1];
    // labels and values; the text labels enter the table
    for (uint32_t i = tid; i < P; i += nthreads)
    {
        uint64_t lv = FUSE_NO_LABEL, lt = FUSE_NO_LABEL;
        float xv = 0.f, xt = 0.f;
        const float r = __fdiv_rn(1.0f, (float)(p.fusion_k + (uint64_t)(i + 1)));
        if (i < nv)
        {
            lv = (uint64_t)vi[i];
            if (!p.rsf)
                xv = r;
            else
            {
                const float n = fuse_norm(vs[i], vs[0], vs[nv - 1]);
                const float w1 = __fsub_rn(1.0f, p.weight);
                xv = p.direction == -1 ? __fmul_rn(n, w1) : __fmul_rn(__fsub_rn(1.0f, n), w1);
            }
        }
        if (i < nt)
        {
            lt = (uint64_t)ti[i];
            xt = p.rsf ? __fmul_rn(fuse_norm(ts[i], ts[0], ts[nt - 1]), p.weight) : r;
            uint32_t h = (uint32_t)((lt * 0x9E3779B97F4A7C15ull) >> 40) & tmask;
            while (atomicCAS(&s_tab[h], 0u, i + 1) != 0u) // (at most nt <= P of the 2 P slots are ever taken: an empty one is found)
                h = (h + 1) & tmask;
        }
        s_label[i] = lv;
        s_bits[i] = __float_as_uint(xv); // (no entry: 0, the key of an empty slot)
        s_label[P + i] = lt;
        s_bits[P + i] = __float_as_uint(xt);
    }
    __syncthreads();
    // the vector entries: RRF (0 + vector) + text; RSF: text assigns, vector adds
    uint32_t owners = 0;
    for (uint32_t i = tid; i < nv; i += nthreads)
    {
        const uint64_t label = s_label[i];
        const float value = __uint_as_float(s_bits[i]);
        int partner = -1;
        uint32_t h = (uint32_t)((label * 0x9E3779B97F4A7C15ull) >> 40) & tmask;
        for (uint32_t e = s_tab[h]; e != 0u; h = (h + 1) & tmask, e = s_tab[h])
            if (s_label[P + e - 1] == label)
            {
                partner = (int)(e - 1);
                break;
            }
        float score;
        if (p.rsf)
            score = partner >= 0 ? __fadd_rn(__uint_as_float(s_bits[P + partner]), value) : __fadd_rn(0.0f, value);
        else
            score = partner >= 0 ? __fadd_rn(__fadd_rn(0.0f, value), __uint_as_float(s_bits[P + partner])) : __fadd_rn(0.0f, value);
        if (partner >= 0)
            s_taken[partner] = 1;
        s_bits[i] = fuse_key(score); // (the vector half: nobody reads it in this phase)
        owners++;
    }
    __syncthreads();
    for (uint32_t i = tid; i < nt; i += nthreads)
    {
        if (s_taken[i])
        {
            s_label[P + i] = FUSE_NO_LABEL;
            s_bits[P + i] = 0;
        }
        else
        {
            const float value = __uint_as_float(s_bits[P + i]);
            s_bits[P + i] = fuse_key(p.rsf ? value : __fadd_rn(0.0f, value));
            owners++;
        }
    }
    if (owners)
        atomicAdd(&s_n[2], owners);
    __syncthreads();
    // bitonic sort of the 2 P (label, key) entries, best first
    for (uint32_t k2 = 2; k2 <= N; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1)
        {
            for (uint32_t t = tid; t < P; t += nthreads)
            {
                const uint32_t a = 2 * j * (t / j) + (t & (j - 1)), b = a + j;
                const bool up = (a & k2) == 0;
                const uint64_t la = s_label[a], lb = s_label[b];
                const uint32_t ka = s_bits[a], kb = s_bits[b];
                if (up ? fuse_before(lb, kb, la, ka) : fuse_before(la, ka, lb, kb))
                {
                    s_label[a] = lb;
                    s_label[b] = la;
                    s_bits[a] = kb;
                    s_bits[b] = ka;
                }
            }
            __syncthreads();
        }
    const uint32_t n = s_n[2] < p.topk ? s_n[2] : p.topk;
    if (tid == 0)
        p.n_out[q] = n;
    for (uint32_t r = tid; r < p.topk; r += nthreads)
    {
        p.out_scores[(size_t)q * p.topk + r] = r < n ? fuse_key_score(s_bits[r]) : 0.f;
        p.out_labels[(size_t)q * p.topk + r] = r < n ? (int64_t)s_label[r] : -1;
    }
}

}

using namespace msvs;

extern "C" int msvs_hybrid_fuse_device(int fusion_type, const float * d_vec_dis, const int64_t * d_vec_ids, size_t kv,
                                       const float * d_txt_scores, const int64_t * d_txt_ids, size_t kt, size_t nq, uint64_t fusion_k,
                                       float fusion_weight, int vector_scan_direction, size_t topk, float * d_out_scores,
                                       int64_t * d_out_labels, uint32_t * d_n_out, void * hip_stream)
{
    return guarded([&] {
        if (nq == 0)
            return;
        if (!d_vec_dis || !d_vec_ids || !d_txt_scores || !d_txt_ids || !d_out_scores || !d_out_labels || !d_n_out || topk == 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer or topk = 0");
        if (kv > FUSE_LONG_MAX || kt > FUSE_LONG_MAX || topk > FUSE_LONG_MAX)
            fail(MSVS_ERR_UNSUPPORTED_K, "the device fusion takes lists and a topk of at most %u rows", FUSE_LONG_MAX);
        if (fusion_type != 0 && fusion_type != 1)
            fail(MSVS_ERR_INVALID_ARGUMENT, "fusion_type: 0 = RRF, 1 = RSF");
        FuseParams p{};
        p.vec_dis = d_vec_dis;
        p.vec_ids = d_vec_ids;
        p.txt_scores = d_txt_scores;
        p.txt_ids = d_txt_ids;
        p.kv = (uint32_t)kv;
        p.kt = (uint32_t)kt;
        p.nq = (uint32_t)nq;
        p.topk = (uint32_t)topk;
        p.rsf = fusion_type == 1;
        p.fusion_k = fusion_k == 0 ? 60 : fusion_k;
        p.weight = fusion_weight;
        p.direction = vector_scan_direction;
        p.out_scores = d_out_scores;
        p.out_labels = d_out_labels;
        p.n_out = d_n_out;
        if (kv <= FUSE_MAX && kt <= FUSE_MAX && topk <= 2 * FUSE_MAX)
            hipLaunchKernelGGL(hybrid_fuse_kernel, dim3((unsigned)nq), dim3(2 * FUSE_MAX), 0, reinterpret_cast<hipStream_t>(hip_stream), p);
        else
        {
            uint32_t P = 2 * FUSE_MAX;
            while (P < std::max(kv, kt))
                P *= 2;
            static std::once_flag once; // more than 64 KiB of dynamic LDS needs the attribute raised once
            std::call_once(once, [] {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&hybrid_fuse_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)fuse_long_lds_bytes(FUSE_LONG_MAX));
            });
            hipLaunchKernelGGL(hybrid_fuse_long_kernel, dim3((unsigned)nq), dim3(std::min(P, FUSE_LONG_THREADS)), fuse_long_lds_bytes(P),
                               reinterpret_cast<hipStream_t>(hip_stream), p, P);
        }
        MSVS_HIP(hipGetLastError());
    });
}
