// graph_kernels.hpp -- device code of the graph index (graph_index.hip): the seeded beam search over a fixed-degree
// neighbour graph whose rows live in a row store (row i is label i), and the integer kernels that build such a graph from exact
// neighbour lists.
//
// graph_search_kernel: one block of 256 threads per query, the whole search of include/msvs.h's definition in one launch.
//   LDS image (graph_lds): the query (ld4 x 16 bytes, staged once) | beam keys (256 x 8) | staged new keys (256 x 8) | expanded
//   flags (256 x 4) | labels to score (256 x 4) | control words (16 x 4) | the visited table (tab x 4).
//   A round takes at most 256 candidate labels, one per thread (the seeds; later the width x R neighbour words of the parents):
//     1. visit: atomicCAS into the open-addressing table; the thread whose CAS wins owns the label, a duplicate loses and is dropped.
//        Winners are compacted into the score list by one LDS atomic per wavefront (their order there reaches no result).
//     2. score: sixteen 16-lane groups take the list's labels grp, grp + 16, ...: canonical_row_chain + row16_tree_sum, as refine_kernel,
//        so sixteen 256-byte-contiguous row requests are in flight; make_key (strict admission, NaN never) -> staged key.
//     3. merge by ranking: thread t holds beam[t] and staged[t] in registers.  An old key's rank is t + the staged keys below it, a new
//        key's the beam keys below it (binary search: the beam is sorted) + the staged keys below it (one pass of broadcast reads both
//        ranks share).  After a barrier every key with rank < ef writes itself and its flag to that rank.  No sort, no serial insertion.
//   Between rounds the parents are the first `width` clear flags of the sorted beam: a ballot per wavefront, four words in LDS, and
//   every thread of a parent's R-lane slice finds its parent from them and loads its neighbour word.
//   The table holds at most tab / 2 labels (the launcher sizes it from the search's own bound), so a probe sequence always ends.
//
//
// graph_search_kernel<METRIC, 8>: the same search over 8-bit codes (create's bit_size=8) -- a label is scored against its DECODED row
//   x^_j = fl(vmin[j] + fl(float(code_j) * step[j])), the IVFSQ quantiser (sq_ivf_kernels.hpp) without a centroid.  Visit, merge, parent
//   pick and epilogue are the code above; the score step and the LDS image are its own:
//   LDS image (graph_sq_lds_bytes): the query | vmin | step (lc4 = round_up(dim, 16) / 4 float4 each, zero padded, staged once) | the
//   6 KiB of beam / stage / flags / labels | control words | the visited table.
//   Stored row: lc4 x 4 bytes in sq_layout.hpp's 8-bit order: one 16-byte load inside a whole 256-byte block is the lane's float4
//   columns 64 b + g, + 16, + 32, + 48 (a "unit"); the natural-order tail is one more unit of 32-bit words.  The lane's columns come
//   out in ascending order, so the four component sums, their sum and the 16-lane tree are canonical_row_chain + row16_tree_sum's.
//   score, rows of at most GRAPH_SQ_MULTI_UNITS units (dim <= 1024): a group takes its labels c, c + 16, c + 32, c + 48 of the round
//   at once and requests every unit of all four rows before the first decode -- up to 64 rows and 16 requests a lane in flight per
//   block, a whole width = 1 round in one go.  Longer rows: one row a group, chunks of GRAPH_SQ_LONG_UNITS units double buffered
//   (the next chunk, or the next label's first, is on its way while this one is decoded), as sq_ivf_scan_kernel's wnext.
//
// graph_search_kernel<METRIC, 16>: the same search over binary16 rows (create's bit_size=16) -- a label is scored against x^ = float(h),
//   an exact conversion, so there is no quantiser and the LDS image is the f32 kernel's (graph_lds_bytes(ld4, tab)): the query alone.
//   Stored row (graph_h16_slot): lc4 = round_up(dim, 16) / 4 float4 columns of four halves, 8 bytes each.  Inside a whole block of 32
//   columns (256 bytes) column 32 b + g sits beside column 32 b + g + 16, so ONE 16-byte load of lane g is its two columns of the
//   block (a "unit") and a group's request is 256 contiguous bytes; the tail (< 32 columns) stays in natural order and is one more
//   unit of two 8-byte words.  The lane's columns come out ascending: the sums are canonical_row_chain + row16_tree_sum's.
//   score (graph_score_h16): rows of at most 4 units (dim <= 512): four labels c, c + 16, c + 32, c + 48 of a group at once, every
//   request out before the first v_cvt_f32_f16; at most 8 units (dim <= 1024): two labels at once -- a whole width = 1 round of R = 32;
//   longer rows: one row a group, chunks of GRAPH_H16_LONG_UNITS units double buffered, as the 8-bit form's.  Nothing but the query
//   is read from LDS, and only its ld4 columns: the pad columns of a stored row (zero halves) are skipped, not multiplied.
//
// graph_search_kernel<METRIC, GRAPH_PQ8 | GRAPH_PQ4>: the same search over product-quantised codes (create's pq_m=M) -- a label is
//   scored by M look-ups into a per-query table T[s][j] (include/msvs.h: "Product-quantised rows").  Visit, merge, parent pick and
//   epilogue are the code above; the table build, the score step, the stored row and the LDS image are its own:
//   LDS image (graph_pq_lds_bytes): T (4 x ksub x M bytes, built once per query by graph_pq_build_tables) | the 6 KiB of beam /
//   stage / flags / labels | control words | the visited table.  The query is read from global memory by the table build alone
//   (one address for the whole block: a scalar load) and has no LDS image.
//   Stored row (GraphPqLayout): sixteen lane slots of W = 4 or 8 bytes, row-major, 64 or 128 bytes a row.  Slot g holds the codes of
//   the sub-spaces g c .. g c + c - 1, c = ceil(M / 16), in ascending order from bit 0 (4 bits: two a byte, a slot starts a byte),
//   zero padded.  One label's codes are ONE aligned 4- or 8-byte load a lane, 64 or 128 contiguous bytes a 16-lane group, and the
//   lane's run -- the partial sum p_g of the definition -- is contiguous in what it loaded.
//   score: a group takes its labels c0, c0 + 16, c0 + 32, c0 + 48 of the round at once and requests all four rows before the first
//   look-up (64 rows in flight a block: a whole width = 1 round of R <= 64); then c look-ups a lane, row16_tree_sum, make_key.
//
// graph_wide_search_kernel<METRIC, BITS, E>: the same search with ef, k <= 4096 (search_wide): a fixed grid, E beam entries a thread,
//   the visited table in global memory.  Its design stands at the kernel.
// graph_join_kernel: the sub-quadratic build's neighbours-of-neighbours join (create's join_iters >= 1), one block per node; it shares
//   graph_visit, graph_wave_place and graph_merge with the search.  Its design stands at the kernel.
// graph_prune_kernel, graph_count_kernel, graph_scan_kernel, graph_scatter_kernel, graph_reverse_kernel: the build, integers only.
// The coded form's quantiser and codes are made by sq_ivf_kernels.hpp's sq_range_kernel / sq_encode_kernel<8> fed a zero centroid.
#pragma once

#include "mfma_scan_kernels.hpp"
#include "pq_ivf_kernels.hpp"
#include "scan_kernels.hpp"
#include "sq_ivf_kernels.hpp"

#pragma clang fp contract(off)

namespace msvs
{

constexpr uint32_t GRAPH_EMPTY = 0xFFFFFFFFu; // no edge / a free slot of the visited table
constexpr uint32_t GRAPH_ROUND = 256;         // candidates of a round at most: min(nprobe, nlist) seeds, width x R neighbour words
constexpr uint32_t GRAPH_CTL = 16;            // control words
// The coded score step's switch point, from the compiler's resource report (gfx950): with four rows of 4 units held
// (64 VGPRs of codes) the kernel takes 119 VGPRs, the f32 kernel's 4 waves per SIMD, no scratch; 6 units a row take 151 VGPRs
// (3 waves), 8 take 184 (2 waves).
constexpr uint32_t GRAPH_SQ_MULTI_UNITS = 4; // rows of up to 4 units (dim <= 1024): four labels a group at once
constexpr uint32_t GRAPH_SQ_LONG_UNITS = 4;  // longer rows: units of a double-buffered chunk

// The kernels' BITS axis: 32 (f32 rows), 16 (binary16 rows), 8 (scalar-quantised codes), and the two product-quantised forms
constexpr int GRAPH_PQ8 = 0x108, GRAPH_PQ4 = 0x104;
constexpr bool graph_is_pq(int bits) { return bits == GRAPH_PQ8 || bits == GRAPH_PQ4; }

struct GraphSearchParams
{
    const float4 * rows;    // n x ld4 at least, zero padded; HBM or mapped pinned host memory
    const float4 * Q;       // nq x ld4, zero padded (normalised for cosine)
    const uint32_t * nbr;   // n x R
    const int32_t * seed;   // nlist
    const int32_t * probes; // nq x P list ids, canonical order, -1 padded
    const uint64_t * alive; // nullable filter bitmap over labels
    int64_t * out_ids;      // nq x k
    float * out_dis;        // nq x k
    uint32_t nbits, n, ld4, R, lgR, ef, k, width, max_iters, P, tab;
    int cosine;
    // BITS 8 (rows is not read):
    const uint4 * codes;         // n x lc4 / 4 16-byte words, stored order (sq_layout.hpp)
    const float4 * vmin, * step; // lc4, zero padded
    uint32_t lc4;                // round_up(dim, 16) / 4 >= ld4
    // BITS 16 (rows, vmin and step are not read): codes is n x lc4 / 2 16-byte words in graph_h16_slot's order
    // BITS GRAPH_PQ8 / GRAPH_PQ4 (rows is not read; codes: n rows of GraphPqLayout, 16 x pq_w bytes each):
    const float * pq_cb;          // the codebooks in pq_cb_index's order
    uint32_t pq_m, pq_dsub, pq_c; // sub-spaces, floats of one, sub-spaces a lane: ceil(pq_m / 16)
    uint32_t pq_w;                // bytes of a lane slot: 4 or 8
};

inline size_t graph_lds_bytes(uint32_t ld4, uint32_t tab)
{
    return (size_t)ld4 * 16 + GRAPH_ROUND * (8 + 8 + 4 + 4) + GRAPH_CTL * 4 + (size_t)tab * 4;
}

/// the coded image: vmin and step beside the query, all three of lc4 float4
inline size_t graph_sq_lds_bytes(uint32_t lc4, uint32_t tab) { return graph_lds_bytes(lc4, tab) + (size_t)lc4 * 32; }

/// The product-quantised stored row: sixteen lane slots of w bytes; slot g holds the codes of the sub-spaces g c .. g c + c - 1
/// from bit 0 up.  pos(s): the byte of a row code s lives in (4 bits: its nibble is (s % c) & 1); row_bytes = 16 w <= 128.
struct GraphPqLayout
{
    uint32_t m, bits, c, w;
    __host__ __device__ GraphPqLayout(uint32_t m_, uint32_t bits_) : m(m_), bits(bits_), c((m_ + 15) / 16), w(((m_ + 15) / 16) * bits_ > 32 ? 8 : 4) {}
    __host__ __device__ uint32_t row_bytes() const { return 16 * w; }
    __host__ __device__ uint32_t pos(uint32_t s) const { return (s / c) * w + (s % c) * bits / 8; }
    __host__ __device__ uint32_t shift(uint32_t s) const { return bits == 4 ? ((s % c) & 1) * 4 : 0; }
};

/// the product-quantised image: the tables where the other forms keep the query
inline size_t graph_pq_lds_bytes(uint32_t m, uint32_t bits, uint32_t tab) { return graph_lds_bytes(m << (bits - 2), tab); }

struct GraphLds
{
    float4 * qs, * vm, * st; // (vm, st: BITS 8; the product-quantised forms: qs is the tables T[s][j], ksub x m floats)
    uint64_t * beam, * stage;
    uint32_t * flag, * slab, * ctl, * table;
    // ctl: 0 labels to score this round, 1 |V|, 2 beam entries, 3 newly admitted keys, 4 alive results; 8 .. 15 four 64-bit ballots
};

/// the slot of the visited table a label's probe sequence starts at
__device__ __forceinline__ uint32_t graph_home(const uint32_t label, const uint32_t tab) { return __umulhi(label * 0x9E3779B1u, tab); }

/// label -> true if this thread is the one that put it into the visited table
__device__ __forceinline__ bool graph_visit(uint32_t * table, const uint32_t tab, const uint32_t label)
{
    uint32_t h = graph_home(label, tab);
    for (;;)
    {
        const uint32_t prev = atomicCAS(&table[h], GRAPH_EMPTY, label);
        if (prev == GRAPH_EMPTY)
            return true;
        if (prev == label)
            return false;
        h = h + 1 == tab ? 0 : h + 1;
    }
}

/// the wavefront's lanes with `pred` get consecutive places behind *counter (one atomic per wavefront) -> this lane's place
__device__ __forceinline__ uint32_t graph_wave_place(uint32_t * counter, const bool pred, const uint32_t lane)
{
    const uint64_t b = __ballot(pred);
    uint32_t base = 0;
    if (lane == 0 && b)
        base = atomicAdd(counter, (uint32_t)__popcll(b));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + (uint32_t)__popcll(b & ((1ull << lane) - 1));
}

/// score, f32 rows: group grp takes the list's labels grp, grp + 16, ... against the row store
template <int METRIC>
__device__ __forceinline__ void graph_score_rows(const GraphSearchParams & a, const GraphLds & L, const uint32_t m, const uint32_t grp, const uint32_t g)
{
    const uint32_t jfull = a.ld4 >> 4, jtail = a.ld4 & 15;
    for (uint32_t c = grp; c < m; c += 16)
    {
        uint32_t id = L.slab[c]; // uniform over the 16 lanes that own slot c
        const float4 acc = canonical_row_chain<METRIC>(a.rows + (size_t)id * a.ld4 + g, L.qs + g, jfull, jtail, g, nullptr, id);
        float s = __fadd_rn(__fadd_rn(acc.x, acc.y), __fadd_rn(acc.z, acc.w));
        s = row16_tree_sum(s);
        if (g == 0)
            L.stage[c] = make_key<METRIC>(s, id);
    }
}

/// unit u of a stored row of nb whole blocks and tc tail columns: a block -> the lane's 16 bytes of it; the tail -> one 32-bit word
/// per float4 column the lane owns there (0 beyond the row), in the block's order of columns
__device__ __forceinline__ uint4 graph_sq_load_unit(const uint4 * row, const uint32_t u, const uint32_t nb, const uint32_t tc, const uint32_t g)
{
    if (u < nb)
        return row[u * 16 + g];
    const uint32_t * tail = reinterpret_cast<const uint32_t *>(row) + nb * 64;
    uint4 v;
    v.x = g < tc ? tail[g] : 0u;
    v.y = g + 16 < tc ? tail[g + 16] : 0u;
    v.z = g + 32 < tc ? tail[g + 32] : 0u;
    v.w = g + 48 < tc ? tail[g + 48] : 0u;
    return v;
}

/// four codes (one float4 column) -> the decoded column: fl(vmin + fl(float(code) * step))
__device__ __forceinline__ float4 graph_sq_decode(const uint32_t w, const float4 m, const float4 s)
{
    float4 y;
    y.x = __fadd_rn(m.x, __fmul_rn((float)(w & 255u), s.x));
    y.y = __fadd_rn(m.y, __fmul_rn((float)((w >> 8) & 255u), s.y));
    y.z = __fadd_rn(m.z, __fmul_rn((float)((w >> 16) & 255u), s.z));
    y.w = __fadd_rn(m.w, __fmul_rn((float)(w >> 24), s.w));
    return y;
}

/// the lane's four columns of unit u, decoded and accumulated in ascending order (padding columns decode to 0 against a 0 query)
template <int METRIC>
__device__ __forceinline__ void graph_sq_score_unit(float4 & acc, const GraphLds & L, const uint4 cw, const uint32_t u, const uint32_t lc4, const uint32_t g)
{
    const uint32_t words[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
        const uint32_t col = u * 64 + g + 16 * e;
        if (col < lc4)
            canonical_update<METRIC>(acc, L.qs[col], graph_sq_decode(words[e], L.vm[col], L.st[col]));
    }
}

template <int METRIC>
__device__ __forceinline__ uint64_t graph_sq_key(const float4 acc, const uint32_t id)
{
    const float s = __fadd_rn(__fadd_rn(acc.x, acc.y), __fadd_rn(acc.z, acc.w));
    return make_key<METRIC>(row16_tree_sum(s), id);
}

/// score, 8-bit codes: the list's labels against their decoded rows (the header's two forms; nu is uniform over the block)
template <int METRIC>
__device__ __forceinline__ void graph_score_codes(const GraphSearchParams & a, const GraphLds & L, const uint32_t m, const uint32_t grp, const uint32_t g)
{
    const uint32_t lc4 = a.lc4, ld16 = lc4 >> 2, nb = lc4 >> 6, tc = lc4 & 63, nu = nb + (tc ? 1 : 0);
    if (nu <= GRAPH_SQ_MULTI_UNITS)
    {
        for (uint32_t c0 = grp; c0 < m; c0 += 64)
        {
            uint4 w[4][GRAPH_SQ_MULTI_UNITS];
            uint32_t id[4];
#pragma unroll
            for (int r = 0; r < 4; r++) // every request of the group's four rows leaves before the first decode
            {
                const uint32_t c = c0 + 16 * r;
                id[r] = c < m ? L.slab[c] : GRAPH_EMPTY;
                const uint4 * row = a.codes + (size_t)id[r] * ld16;
#pragma unroll
                for (uint32_t u = 0; u < GRAPH_SQ_MULTI_UNITS; u++)
                {
                    w[r][u] = make_uint4(0, 0, 0, 0);
                    if (id[r] != GRAPH_EMPTY && u < nu)
                        w[r][u] = graph_sq_load_unit(row, u, nb, tc, g);
                }
            }
            // row after row (the four rows side by side, one LDS read of query, vmin and step serving all of them, measured slower:
            // 129 VGPRs, 3 waves, and 3 - 5 % more time at every shape of DESIGN.md 4.14's table)
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (id[r] != GRAPH_EMPTY)
                {
                    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (uint32_t u = 0; u < GRAPH_SQ_MULTI_UNITS; u++)
                        if (u < nu)
                            graph_sq_score_unit<METRIC>(acc, L, w[r][u], u, lc4, g);
                    const uint64_t key = graph_sq_key<METRIC>(acc, id[r]);
                    if (g == 0)
                        L.stage[c0 + 16 * r] = key;
                }
        }
        return;
    }
    uint4 next[GRAPH_SQ_LONG_UNITS];
    auto load_chunk = [&](const uint32_t id, const uint32_t u0) {
        const uint4 * row = a.codes + (size_t)id * ld16;
#pragma unroll
        for (uint32_t e = 0; e < GRAPH_SQ_LONG_UNITS; e++)
        {
            next[e] = make_uint4(0, 0, 0, 0);
            if (u0 + e < nu)
                next[e] = graph_sq_load_unit(row, u0 + e, nb, tc, g);
        }
    };
    if (grp < m)
        load_chunk(L.slab[grp], 0);
    for (uint32_t c = grp; c < m; c += 16)
    {
        const uint32_t id = L.slab[c];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t u0 = 0; u0 < nu; u0 += GRAPH_SQ_LONG_UNITS)
        {
            uint4 cur[GRAPH_SQ_LONG_UNITS];
#pragma unroll
            for (uint32_t e = 0; e < GRAPH_SQ_LONG_UNITS; e++)
                cur[e] = next[e];
            if (u0 + GRAPH_SQ_LONG_UNITS < nu)
                load_chunk(id, u0 + GRAPH_SQ_LONG_UNITS);
            else if (c + 16 < m)
                load_chunk(L.slab[c + 16], 0);
#pragma unroll
            for (uint32_t e = 0; e < GRAPH_SQ_LONG_UNITS; e++)
                if (u0 + e < nu)
                    graph_sq_score_unit<METRIC>(acc, L, cur[e], u0 + e, lc4, g);
        }
        const uint64_t key = graph_sq_key<METRIC>(acc, id);
        if (g == 0)
            L.stage[c] = key;
    }
}

// ------------------------------------------------------------------------------------------- binary16 rows

// The score step's forms, from the compiler's resource report (gfx950): ROWS x UNITS 16-byte words are held while a
// group's rows are scored -- 4 x 4 and 2 x 8 are 64 VGPRs of halves; the long form holds two chunks of GRAPH_H16_LONG_UNITS.  The
// narrow kernel takes 111 VGPRs, the wide one 126 / 128 at E = 1 / 2: 4 waves per SIMD, no scratch.  At E = 4 / 8 the wide kernel
// with 64 VGPRs of halves took 130 / 134 (3 waves); LIGHT halves the rows at once (2 x 4, 1 x 8): 102 / 106.  E = 16: 146, as f32's 149.
constexpr uint32_t GRAPH_H16_LONG_UNITS = 4;

/// The binary16 stored row of lc4 float4 columns (four halves, 8 bytes each): slot(c) = the 8-byte word of natural column c, col(s)
/// its inverse.  Inside a whole block of 32 columns the words of columns 32 b + g and 32 b + g + 16 are adjacent (2 g, 2 g + 1);
/// the tail keeps its order.  Half j of a row lives at half 4 slot(j / 4) + j % 4 (sq_layout.hpp's sq16_stored_pos).
__host__ __device__ inline uint32_t graph_h16_slot(const uint32_t c, const uint32_t lc4)
{
    return c >= (lc4 & ~31u) ? c : (c & ~31u) + ((c & 15u) << 1) + ((c >> 4) & 1u);
}
__host__ __device__ inline uint32_t graph_h16_col(const uint32_t s, const uint32_t lc4)
{
    return s >= (lc4 & ~31u) ? s : (s & ~31u) + ((s & 31u) >> 1) + ((s & 1u) << 4);
}

/// X: n rows of ld4 float4 (zero padded; HBM or mapped pinned host memory) -> n stored binary16 rows; a thread an 8-byte word.
/// (_Float16)x is v_cvt_f16_f32 in the default modes: to nearest even, subnormals kept, overflow to +-inf, NaN stays NaN.
static __global__ __launch_bounds__(BLOCK) void graph_h16_encode_kernel(const float4 * X, size_t n, uint32_t ld4, uint32_t lc4, uint2 * out)
{
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n * lc4)
        return;
    const size_t r = i / lc4;
    const uint32_t c = graph_h16_col((uint32_t)(i - r * lc4), lc4);
    const float4 x = c < ld4 ? X[r * ld4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    half2v lo, hi;
    lo[0] = (_Float16)x.x;
    lo[1] = (_Float16)x.y;
    hi[0] = (_Float16)x.z;
    hi[1] = (_Float16)x.w;
    out[i] = make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi));
}

/// unit u of a stored row of nb whole blocks and tc tail columns: the lane's columns 32 u + g (x, y) and 32 u + g + 16 (z, w); a block
/// is one 16-byte load, the tail one 8-byte word per column the lane owns there (0 beyond the row)
__device__ __forceinline__ uint4 graph_h16_load_unit(const uint4 * row, const uint32_t u, const uint32_t nb, const uint32_t tc, const uint32_t g)
{
    if (u < nb)
        return row[u * 16 + g];
    const uint2 * tail = reinterpret_cast<const uint2 *>(row) + nb * 32;
    const uint2 zero = make_uint2(0u, 0u), a = g < tc ? tail[g] : zero, b = g + 16 < tc ? tail[g + 16] : zero;
    return make_uint4(a.x, a.y, b.x, b.y);
}

/// four halves (one float4 column) -> the decoded column, exactly: two packed pairs, four v_cvt_f32_f16
__device__ __forceinline__ float4 graph_h16_decode(const uint32_t w0, const uint32_t w1)
{
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const half2v lo = __builtin_bit_cast(half2v, w0), hi = __builtin_bit_cast(half2v, w1);
    return make_float4((float)lo[0], (float)lo[1], (float)hi[0], (float)hi[1]);
}

/// the lane's two columns of unit u, decoded and accumulated in ascending order; the query has ld4 columns, a row's pad columns none
template <int METRIC>
__device__ __forceinline__ void graph_h16_score_unit(float4 & acc, const float4 * qs, const uint4 w, const uint32_t u, const uint32_t ld4, const uint32_t g)
{
    const uint32_t col = u * 32 + g;
    if (col < ld4)
        canonical_update<METRIC>(acc, qs[col], graph_h16_decode(w.x, w.y));
    if (col + 16 < ld4)
        canonical_update<METRIC>(acc, qs[col + 16], graph_h16_decode(w.z, w.w));
}

/// rows of at most UNITS units: a group takes ROWS labels c0, c0 + 16, ... of the round at once; every request leaves before the
/// first convert, then row after row
template <int METRIC, int ROWS, int UNITS>
__device__ __forceinline__ void graph_h16_score_multi(const GraphSearchParams & a, const GraphLds & L, const uint32_t m, const uint32_t grp, const uint32_t g,
                                                      const uint32_t nb, const uint32_t tc, const uint32_t nu)
{
    const uint32_t ld16 = a.lc4 >> 1;
    for (uint32_t c0 = grp; c0 < m; c0 += 16 * ROWS)
    {
        uint4 w[ROWS][UNITS];
        uint32_t id[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++)
        {
            const uint32_t c = c0 + 16 * r;
            id[r] = c < m ? L.slab[c] : GRAPH_EMPTY;
            const uint4 * row = a.codes + (size_t)id[r] * ld16;
#pragma unroll
            for (uint32_t u = 0; u < UNITS; u++)
            {
                w[r][u] = make_uint4(0, 0, 0, 0);
                if (id[r] != GRAPH_EMPTY && u < nu)
                    w[r][u] = graph_h16_load_unit(row, u, nb, tc, g);
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; r++)
            if (id[r] != GRAPH_EMPTY) // (uniform over the group)
            {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (uint32_t u = 0; u < UNITS; u++)
                    if (u < nu)
                        graph_h16_score_unit<METRIC>(acc, L.qs, w[r][u], u, a.ld4, g);
                const uint64_t key = graph_sq_key<METRIC>(acc, id[r]);
                if (g == 0)
                    L.stage[c0 + 16 * r] = key;
            }
    }
}

/// score, binary16 rows: the list's labels against their decoded rows (the header's three forms; nu is uniform over the block)
template <int METRIC, bool LIGHT = false>
__device__ __forceinline__ void graph_score_h16(const GraphSearchParams & a, const GraphLds & L, const uint32_t m, const uint32_t grp, const uint32_t g)
{
    const uint32_t nb = a.lc4 >> 5, tc = a.lc4 & 31, nu = nb + (tc ? 1 : 0), ld16 = a.lc4 >> 1;
    if (nu <= 4)
        return graph_h16_score_multi<METRIC, LIGHT ? 2 : 4, 4>(a, L, m, grp, g, nb, tc, nu);
    if (nu <= 8)
        return graph_h16_score_multi<METRIC, LIGHT ? 1 : 2, 8>(a, L, m, grp, g, nb, tc, nu);
    uint4 next[GRAPH_H16_LONG_UNITS];
    auto load_chunk = [&](const uint32_t id, const uint32_t u0) {
        const uint4 * row = a.codes + (size_t)id * ld16;
#pragma unroll
        for (uint32_t e = 0; e < GRAPH_H16_LONG_UNITS; e++)
        {
            next[e] = make_uint4(0, 0, 0, 0);
            if (u0 + e < nu)
                next[e] = graph_h16_load_unit(row, u0 + e, nb, tc, g);
        }
    };
    if (grp < m)
        load_chunk(L.slab[grp], 0);
    for (uint32_t c = grp; c < m; c += 16)
    {
        const uint32_t id = L.slab[c];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint32_t u0 = 0; u0 < nu; u0 += GRAPH_H16_LONG_UNITS)
        {
            uint4 cur[GRAPH_H16_LONG_UNITS];
#pragma unroll
            for (uint32_t e = 0; e < GRAPH_H16_LONG_UNITS; e++)
                cur[e] = next[e];
            if (u0 + GRAPH_H16_LONG_UNITS < nu) // the next chunk, or the next label's first, is on its way during the converts
                load_chunk(id, u0 + GRAPH_H16_LONG_UNITS);
            else if (c + 16 < m)
                load_chunk(L.slab[c + 16], 0);
#pragma unroll
            for (uint32_t e = 0; e < GRAPH_H16_LONG_UNITS; e++)
                if (u0 + e < nu)
                    graph_h16_score_unit<METRIC>(acc, L.qs, cur[e], u0 + e, a.ld4, g);
        }
        const uint64_t key = graph_sq_key<METRIC>(acc, id);
        if (g == 0)
            L.stage[c] = key;
    }
}

// ------------------------------------------------------------------------------------------- product-quantised rows

/// T[s][j] of include/msvs.h for the query q (dim floats in global memory, normalised for cosine), into LDS; the caller's barrier
/// follows.  8 bits: thread j owns entry j of every sub-space, so a wavefront's codebook loads are 256 contiguous bytes and q's
/// element is one address for the block.  4 bits: a wavefront is (4 consecutive sub-spaces) x (16 entries), pq_cb_index's grouped
/// order; the block takes 16 sub-spaces a pass.
template <int METRIC, int BITS>
__device__ __forceinline__ void graph_pq_build_tables(const GraphSearchParams & a, float * lut, const float * q, const uint32_t tid)
{
    const uint32_t m = a.pq_m, dsub = a.pq_dsub;
    auto term = [](const float qv, const float v) {
        if constexpr (METRIC == M_L2)
        {
            const float df = __fsub_rn(qv, v);
            return __fmul_rn(df, df);
        }
        else
            return __fmul_rn(qv, v);
    };
    if constexpr (BITS == GRAPH_PQ8)
    {
        // pq_cb_index<8>(s, t, tid, ...) = (s dsub + t) 256 + tid: the columns i = s dsub + t are one run of dim loads, taken eight
        // at a time so that eight requests a thread are in flight; a table entry is closed whenever its dsub terms are in
        const float * cb = a.pq_cb + tid;
        const uint32_t dim = m * dsub;
        uint32_t s = 0, t = 0;
        float e = 0.f;
        for (uint32_t i0 = 0; i0 < dim; i0 += 8)
        {
            float v[8];
#pragma unroll
            for (uint32_t u = 0; u < 8; u++)
                v[u] = i0 + u < dim ? cb[(size_t)(i0 + u) * 256] : 0.f;
#pragma unroll
            for (uint32_t u = 0; u < 8; u++)
                if (i0 + u < dim)
                {
                    e = __fadd_rn(e, term(q[i0 + u], v[u]));
                    if (++t == dsub)
                    {
                        lut[s * 256 + tid] = e;
                        e = 0.f;
                        t = 0;
                        s++;
                    }
                }
        }
    }
    else
    {
        const uint32_t j = tid & 15;
        for (uint32_t s = tid >> 4; s < m; s += 16)
        {
            const float * cb = a.pq_cb + pq_cb_index<4>(s, 0, j, m, dsub);
            const uint32_t gw = pq_cb_stride<4>(s, m);
            const float * qs = q + s * dsub;
            float e = 0.f;
            for (uint32_t t = 0; t < dsub; t++)
                e = __fadd_rn(e, term(qs[t], cb[(size_t)t * gw]));
            lut[s * 16 + j] = e;
        }
    }
}

/// score, product-quantised codes: lane g of the group that owns a label adds its run's table entries in ascending order (the
/// definition's p_g); the sixteen partials fold with row16_tree_sum.  The loads of the group's four labels leave before the first
/// look-up.  w64: the lane's slot, codes from bit 0 up.
template <int METRIC, int BITS>
__device__ __forceinline__ void graph_score_pq(const GraphSearchParams & a, const GraphLds & L, const uint32_t m, const uint32_t grp, const uint32_t g)
{
    constexpr uint32_t CB = BITS == GRAPH_PQ8 ? 8 : 4, KSUB = 1u << CB;
    const float * lut = reinterpret_cast<const float *>(L.qs);
    const uint32_t c = a.pq_c, s0 = g * c, run = s0 < a.pq_m ? min(c, a.pq_m - s0) : 0u, words = a.pq_w >> 2;
    const uint32_t * codes = reinterpret_cast<const uint32_t *>(a.codes);
    for (uint32_t c0 = grp; c0 < m; c0 += 64)
    {
        uint64_t w[4];
        uint32_t id[4];
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            const uint32_t cc = c0 + 16 * r;
            id[r] = cc < m ? L.slab[cc] : GRAPH_EMPTY;
            w[r] = 0;
            if (id[r] != GRAPH_EMPTY)
            {
                const uint32_t * slot = codes + ((size_t)id[r] * 16 + g) * words;
                if (words == 2)
                {
                    const uint2 v = *reinterpret_cast<const uint2 *>(slot);
                    w[r] = (uint64_t)v.y << 32 | v.x;
                }
                else
                    w[r] = *slot;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (id[r] != GRAPH_EMPTY) // (uniform over the group)
            {
                // c steps for every lane, so the group stays in step up to the lane sum; a step past the lane's run reads the
                // last table (a pad code is 0) and is dropped by a select
                float p = 0.f;
                uint64_t v = w[r];
                for (uint32_t i = 0; i < c; i++, v >>= CB)
                {
                    const float e = lut[min(s0 + i, a.pq_m - 1) * KSUB + ((uint32_t)v & (KSUB - 1))];
                    p = i < run ? __fadd_rn(p, e) : p;
                }
                p = row16_tree_sum(p);
                if (g == 0)
                    L.stage[c0 + 16 * r] = make_key<METRIC>(p, id[r]);
            }
    }
}

/// the encoders' rows (pq_encode_kernel: a code a byte; pq4_encode_kernel: two a byte; rows of mp bytes) -> the stored rows of
/// GraphPqLayout, a thread a stored byte, pad bits 0
static __global__ void graph_pq_repack_kernel(const uint8_t * src, size_t n, uint32_t m, uint32_t bits, uint32_t mp, uint8_t * dst)
{
    const GraphPqLayout lay(m, bits);
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * lay.row_bytes())
        return;
    const size_t r = e / lay.row_bytes();
    const uint32_t b = (uint32_t)(e - r * lay.row_bytes()), g = b / lay.w, o = b % lay.w;
    uint32_t out = 0;
    for (uint32_t h = 0; h < 8 / bits; h++) // the codes of this byte
    {
        const uint32_t i = o * (8 / bits) + h, s = g * lay.c + i;
        if (i < lay.c && s < m)
            out |= (bits == 8 ? src[r * mp + s] : (src[r * mp + (s >> 1)] >> ((s & 1) * 4)) & 15u) << (h * bits);
    }
    dst[e] = (uint8_t)out;
}

/// Merge by ranking: the m staged keys go into the sorted beam of cnt keys, cut to ef.  Entered with every thread past the barrier
/// behind the last staged key; left past a barrier with ctl[2] the beam's new fill, ctl[1] grown by m and ctl[0] = ctl[3] = 0.
__device__ __forceinline__ void graph_merge(const GraphLds & L, const uint32_t ef, const uint32_t m, const uint32_t cnt, const uint32_t tid)
{
    const uint32_t lane = tid & 63;
    const uint64_t old = tid < cnt ? L.beam[tid] : KEY_NONE, neu = tid < m ? L.stage[tid] : KEY_NONE;
    const uint32_t old_flag = tid < cnt ? L.flag[tid] : 0;
    uint32_t rank_old = tid, rank_new = 0;
    for (uint32_t j = 0; j < m; j++)
    {
        const uint64_t kj = L.stage[j]; // one address for the whole block: a broadcast read
        rank_old += kj < old ? 1u : 0u;
        rank_new += kj < neu ? 1u : 0u;
    }
    if (neu != KEY_NONE)
    {
        uint32_t lo = 0, hi = cnt; // beam keys below neu
        while (lo < hi)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (L.beam[mid] < neu)
                lo = mid + 1;
            else
                hi = mid;
        }
        rank_new += lo;
    }
    (void)graph_wave_place(&L.ctl[3], neu != KEY_NONE, lane);
    __syncthreads(); // everybody has read the beam, the flags and the staged keys
    if (old != KEY_NONE && rank_old < ef)
    {
        L.beam[rank_old] = old;
        L.flag[rank_old] = old_flag;
    }
    if (neu != KEY_NONE && rank_new < ef)
    {
        L.beam[rank_new] = neu;
        L.flag[rank_new] = 0;
    }
    const uint32_t admitted = L.ctl[3];
    __syncthreads();
    if (tid == 0)
    {
        L.ctl[2] = min(ef, cnt + admitted);
        L.ctl[1] += m;
        L.ctl[0] = 0;
        L.ctl[3] = 0;
    }
    __syncthreads();
}

/// One round: this thread's candidate label (GRAPH_EMPTY: none) is visited, the winners are scored and merged into the beam.
/// Entered and left with every thread past a barrier and ctl[0] = ctl[3] = 0.
template <int METRIC, int BITS>
__device__ __forceinline__ void graph_round(const GraphSearchParams & a, const GraphLds & L, const uint32_t lab, const uint32_t tid)
{
    const uint32_t lane = tid & 63, grp = tid >> 4, g = tid & 15;
    const bool won = lab != GRAPH_EMPTY && graph_visit(L.table, a.tab, lab);
    const uint32_t place = graph_wave_place(&L.ctl[0], won, lane);
    if (won)
        L.slab[place] = lab;
    __syncthreads();
    const uint32_t m = L.ctl[0], cnt = L.ctl[2];
    if constexpr (BITS == 8)
        graph_score_codes<METRIC>(a, L, m, grp, g);
    else if constexpr (BITS == 16)
        graph_score_h16<METRIC>(a, L, m, grp, g);
    else if constexpr (graph_is_pq(BITS))
        graph_score_pq<METRIC, BITS>(a, L, m, grp, g);
    else
        graph_score_rows<METRIC>(a, L, m, grp, g);
    __syncthreads();
    graph_merge(L, a.ef, m, cnt, tid);
}

/// bytes of the image before the beam: the query (| vmin | step), or the product-quantised tables
template <int BITS>
__device__ __forceinline__ size_t graph_head_bytes(const GraphSearchParams & a)
{
    if constexpr (graph_is_pq(BITS))
        return (size_t)a.pq_m * 4 << (BITS & 15);
    return BITS == 8 ? (size_t)a.lc4 * 48 : (size_t)a.ld4 * 16;
}

template <int METRIC, int BITS = 32>
static __global__ __launch_bounds__(BLOCK) void graph_search_kernel(const GraphSearchParams a)
{
    static_assert(BITS == 32 || BITS == 16 || BITS == 8 || graph_is_pq(BITS), "f32 rows of a row store, binary16 rows, 8-bit codes, or product-quantised codes");
    extern __shared__ __align__(16) unsigned char graph_lds[];
    GraphLds L;
    L.qs = reinterpret_cast<float4 *>(graph_lds);
    L.vm = L.qs + a.lc4;
    L.st = L.vm + a.lc4;
    L.beam = reinterpret_cast<uint64_t *>(graph_lds + graph_head_bytes<BITS>(a));
    L.stage = L.beam + GRAPH_ROUND;
    L.flag = reinterpret_cast<uint32_t *>(L.stage + GRAPH_ROUND);
    L.slab = L.flag + GRAPH_ROUND;
    L.ctl = L.slab + GRAPH_ROUND;
    L.table = L.ctl + GRAPH_CTL;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (BITS == 8)
        for (uint32_t i = tid; i < a.lc4; i += BLOCK)
        {
            L.qs[i] = i < a.ld4 ? a.Q[(size_t)q * a.ld4 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
            L.vm[i] = a.vmin[i];
            L.st[i] = a.step[i];
        }
    else if constexpr (graph_is_pq(BITS))
        graph_pq_build_tables<METRIC, BITS>(a, reinterpret_cast<float *>(L.qs), reinterpret_cast<const float *>(a.Q + (size_t)q * a.ld4), tid);
    else
        for (uint32_t i = tid; i < a.ld4; i += BLOCK)
            L.qs[i] = a.Q[(size_t)q * a.ld4 + i];
    for (uint32_t i = tid; i < a.tab; i += BLOCK)
        L.table[i] = GRAPH_EMPTY;
    if (tid < GRAPH_CTL)
        L.ctl[tid] = 0;
    __syncthreads();
    // the seeds of the probed lists
    uint32_t lab = GRAPH_EMPTY;
    if (tid < a.P)
    {
        const int32_t l = a.probes[(size_t)q * a.P + tid];
        const int32_t s = l >= 0 ? a.seed[l] : -1;
        if (s >= 0 && (uint32_t)s < a.n)
            lab = (uint32_t)s;
    }
    graph_round<METRIC, BITS>(a, L, lab, tid);
    uint64_t * ballots = reinterpret_cast<uint64_t *>(L.ctl + 8);
    const uint32_t fan = a.width << a.lgR;
    for (uint32_t it = 0; it < a.max_iters; it++)
    {
        const uint32_t cnt = L.ctl[2];
        if (L.ctl[1] + fan > MSVS_GRAPH_VISITED_MAX)
            break;
        const uint64_t b = __ballot(tid < cnt && L.flag[tid] == 0);
        if (lane == 0)
            ballots[wave] = b;
        __syncthreads();
        const uint64_t b0 = ballots[0], b1 = ballots[1], b2 = ballots[2], b3 = ballots[3];
        __syncthreads(); // (the next iteration's ballots must not overtake a reader)
        const uint32_t open = (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        if (open == 0)
            break;
        lab = GRAPH_EMPTY;
        const uint32_t p = tid >> a.lgR; // this thread's parent: the p-th clear flag
        if (tid < fan && p < open)
        {
            uint32_t skip = p, base = 0;
            uint64_t w = b0;
            if (skip >= (uint32_t)__popcll(w))
                skip -= (uint32_t)__popcll(w), w = b1, base = 64;
            if (skip >= (uint32_t)__popcll(w))
                skip -= (uint32_t)__popcll(w), w = b2, base = 128;
            if (skip >= (uint32_t)__popcll(w))
                skip -= (uint32_t)__popcll(w), w = b3, base = 192;
            for (; skip; skip--)
                w &= w - 1;
            const uint32_t slot = base + (uint32_t)__builtin_ctzll(w);
            const uint32_t parent = (uint32_t)L.beam[slot], r = tid & (a.R - 1);
            const uint32_t e = a.nbr[(size_t)parent * a.R + r];
            lab = e < a.n ? e : GRAPH_EMPTY;
            if (r == 0)
                L.flag[slot] = 1;
        }
        graph_round<METRIC, BITS>(a, L, lab, tid);
    }
    // the first k alive entries of the beam
    const uint32_t cnt = L.ctl[2];
    const uint64_t key = tid < cnt ? L.beam[tid] : KEY_NONE;
    bool ok = key != KEY_NONE;
    if (ok && a.alive)
    {
        const uint32_t id = (uint32_t)key;
        ok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
    }
    const uint64_t bo = __ballot(ok);
    if (lane == 0)
        ballots[wave] = bo;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < 4; w++)
    {
        const uint32_t c = (uint32_t)__popcll(ballots[w]);
        before += w < wave ? c : 0;
        total += c;
    }
    const uint32_t rank = before + (uint32_t)__popcll(bo & ((1ull << lane) - 1));
    if (ok && rank < a.k)
    {
        const size_t o = (size_t)q * a.k + rank;
        a.out_ids[o] = (int64_t)(uint32_t)key;
        const float v = key_value<METRIC>(key);
        a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
    }
    for (uint32_t i = total + tid; i < a.k; i += BLOCK)
    {
        const size_t o = (size_t)q * a.k + i;
        a.out_ids[o] = -1;
        const float v = key_value<METRIC>(KEY_NONE);
        a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
    }
}

// ------------------------------------------------------------------------------------------- the wide search (ef, k <= 4096)

// graph_wide_search_kernel<METRIC, BITS, E>: the search of include/msvs.h's definition with a beam of up to MSVS_MAX_K_ROUNDS entries
// and a visited set of up to MSVS_GRAPH_WIDE_VISITED_MAX labels.  Visit, score and keys are the narrow search's functions; the rest:
//   Work split: a FIXED grid (the launcher: what fits by LDS image x CUs, and by the table budget); block b serves queries b,
//     b + gridDim.x, ...  BITS 8 stages vmin and step once per block, the query once per query.
//   Visited table: a slice of `tab` words of GLOBAL memory per block, cleared at the start of every query with 16-byte stores; after
//     a fence and a barrier it is touched through atomicCAS alone (graph_visit), so no cached line ever reaches a decision.
//   LDS image (graph_wide_lds_bytes): the query (| vmin | step) | beam keys (ef x 8) | staged keys (256 x 8) | labels to score
//     (256 x 4) | control words (32 x 4) | expanded flags (ef bytes).
//   Merge by ranking, E = the beam entries a thread holds (entry e x 256 + tid; E x 256 >= ef):
//     1. the m <= 256 staged keys rank among themselves (broadcast reads) and are rewritten in rank order, the admitted ones first;
//     2. a thread's E old keys each count the staged keys below them: E independent branch-free binary searches of <= 9 steps;
//        new rank = old position + that count;
//     3. staged key t counts the beam keys below it (<= 13 steps); its rank = that count + t;
//     4. after a barrier every entry with rank < ef writes itself and its flag -- an old entry only if its rank moved.
//   Parent pick: ctl[4] is a cursor before which every beam entry is expanded.  The pick scans windows of 256 entries from it, one
//     ballot per wavefront, until `width` clear flags are found or the fill ends; a merge lowers the cursor to the lowest rank a new
//     key took.  The parents are the `width` lowest-key unexpanded entries, as in the narrow search.
//   Epilogue: the beam in windows of 256 with a running count of alive entries; the first k are written, the rest padded.
constexpr uint32_t GRAPH_WIDE_CTL = 32; // 0 labels to score, 1 |V|, 2 beam entries, 3 admitted keys, 4 cursor; 8 .. 15 ballots; 16 .. 19 parent slots

struct GraphWideParams : GraphSearchParams
{
    uint32_t * tables; // gridDim.x slices of tab words (tab % 4 == 0)
    uint32_t nq;
};

/// q4: the float4 of the query image (ld4; BITS 8: 3 lc4)
inline size_t graph_wide_lds_bytes(uint32_t q4, uint32_t ef)
{
    return (size_t)q4 * 16 + (size_t)ef * 8 + GRAPH_ROUND * (8 + 4) + GRAPH_WIDE_CTL * 4 + (((size_t)ef + 15) & ~(size_t)15);
}

/// sorted keys[0 .. n) -> how many are below key; p2: the largest power of two <= n (0 for n = 0).  No branch: chains interleave.
__device__ __forceinline__ uint32_t graph_count_below(const uint64_t * keys, const uint32_t n, const uint32_t p2, const uint64_t key)
{
    uint32_t pos = 0;
    for (uint32_t s = p2; s; s >>= 1)
        pos += pos + s <= n && keys[pos + s - 1] < key ? s : 0u;
    return pos;
}

__device__ __forceinline__ uint32_t graph_floor_pow2(const uint32_t n) { return n ? 1u << (31 - __builtin_clz(n)) : 0u; }

/// The wide merge (the header's steps 1 - 4).  Entered and left as graph_merge; ctl[4] is lowered to the lowest rank a new key took.
template <int E>
__device__ __forceinline__ void graph_wide_merge(const GraphLds & L, uint8_t * flag, const uint32_t ef, const uint32_t m, const uint32_t cnt,
                                                 const uint32_t tid)
{
    const uint32_t lane = tid & 63;
    // 1. the staged keys in rank order (KEY_NONE: not admitted, behind every key)
    uint64_t neu = tid < m ? L.stage[tid] : KEY_NONE;
    uint32_t rank_new = 0;
    for (uint32_t j = 0; j < m; j++)
        rank_new += L.stage[j] < neu ? 1u : 0u; // one address for the whole block: a broadcast read
    (void)graph_wave_place(&L.ctl[3], neu != KEY_NONE, lane);
    __syncthreads();
    if (neu != KEY_NONE)
        L.stage[rank_new] = neu;
    __syncthreads();
    const uint32_t ma = L.ctl[3], pa = graph_floor_pow2(ma), pc = graph_floor_pow2(cnt);
    // 2. the old keys: position + staged keys below
    uint64_t old[E];
    uint32_t rank_old[E];
    uint8_t old_flag[E];
#pragma unroll
    for (int e = 0; e < E; e++)
    {
        const uint32_t i = (uint32_t)e * BLOCK + tid;
        old[e] = i < cnt ? L.beam[i] : KEY_NONE;
        old_flag[e] = i < cnt ? flag[i] : (uint8_t)0;
        rank_old[e] = 0;
    }
    for (uint32_t s = pa; s; s >>= 1)
#pragma unroll
        for (int e = 0; e < E; e++)
            rank_old[e] += rank_old[e] + s <= ma && L.stage[rank_old[e] + s - 1] < old[e] ? s : 0u;
    // 3. the new keys: beam keys below + staged rank
    neu = tid < ma ? L.stage[tid] : KEY_NONE;
    rank_new = tid < ma ? graph_count_below(L.beam, cnt, pc, neu) + tid : ef;
    uint32_t low = rank_new;
    for (int d = 32; d; d >>= 1)
        low = min(low, (uint32_t)__shfl_xor((int)low, d));
    __syncthreads(); // everybody has read the beam, the flags and the staged keys
    // 4. every survivor writes itself
#pragma unroll
    for (int e = 0; e < E; e++)
    {
        const uint32_t i = (uint32_t)e * BLOCK + tid, r = i + rank_old[e];
        if (old[e] != KEY_NONE && r != i && r < ef)
        {
            L.beam[r] = old[e];
            flag[r] = old_flag[e];
        }
    }
    if (rank_new < ef)
    {
        L.beam[rank_new] = neu;
        flag[rank_new] = 0;
    }
    if (lane == 0 && low < ef)
        atomicMin(&L.ctl[4], low);
    __syncthreads();
    if (tid == 0)
    {
        L.ctl[2] = min(ef, cnt + ma);
        L.ctl[1] += m;
        L.ctl[0] = 0;
        L.ctl[3] = 0;
    }
    __syncthreads();
}

/// graph_round with the visited table in global memory and the wide merge
template <int METRIC, int BITS, int E>
__device__ __forceinline__ void graph_wide_round(const GraphWideParams & a, const GraphLds & L, uint8_t * flag, const uint32_t lab, const uint32_t tid)
{
    const uint32_t lane = tid & 63, grp = tid >> 4, g = tid & 15;
    const bool won = lab != GRAPH_EMPTY && graph_visit(L.table, a.tab, lab);
    const uint32_t place = graph_wave_place(&L.ctl[0], won, lane);
    if (won)
        L.slab[place] = lab;
    __syncthreads();
    const uint32_t m = L.ctl[0], cnt = L.ctl[2];
    if constexpr (BITS == 8)
        graph_score_codes<METRIC>(a, L, m, grp, g);
    else if constexpr (BITS == 16)
        graph_score_h16<METRIC, (E >= 4)>(a, L, m, grp, g);
    else if constexpr (graph_is_pq(BITS))
        graph_score_pq<METRIC, BITS>(a, L, m, grp, g);
    else
        graph_score_rows<METRIC>(a, L, m, grp, g);
    __syncthreads();
    graph_wide_merge<E>(L, flag, a.ef, m, cnt, tid);
}

template <int METRIC, int BITS, int E>
static __global__ __launch_bounds__(BLOCK) void graph_wide_search_kernel(const GraphWideParams a)
{
    static_assert(BITS == 32 || BITS == 16 || BITS == 8 || graph_is_pq(BITS), "f32 rows of a row store, binary16 rows, 8-bit codes, or product-quantised codes");
    static_assert(E * BLOCK <= MSVS_MAX_K_ROUNDS, "the beam's entries a thread holds");
    extern __shared__ __align__(16) unsigned char graph_lds[];
    GraphLds L;
    L.qs = reinterpret_cast<float4 *>(graph_lds);
    L.vm = L.qs + a.lc4;
    L.st = L.vm + a.lc4;
    L.beam = reinterpret_cast<uint64_t *>(graph_lds + graph_head_bytes<BITS>(a));
    L.stage = L.beam + a.ef;
    L.flag = nullptr; // (the wide beam's flags are bytes)
    L.slab = reinterpret_cast<uint32_t *>(L.stage + GRAPH_ROUND);
    L.ctl = L.slab + GRAPH_ROUND;
    L.table = a.tables + (size_t)blockIdx.x * a.tab;
    uint8_t * flag = reinterpret_cast<uint8_t *>(L.ctl + GRAPH_WIDE_CTL);
    uint64_t * ballots = reinterpret_cast<uint64_t *>(L.ctl + 8);
    uint32_t * parents = L.ctl + 16;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fan = a.width << a.lgR;
    if constexpr (BITS == 8)
        for (uint32_t i = tid; i < a.lc4; i += BLOCK)
        {
            L.vm[i] = a.vmin[i];
            L.st[i] = a.step[i];
        }
    for (uint32_t q = blockIdx.x; q < a.nq; q += gridDim.x)
    {
        __syncthreads(); // the previous query's last reader is done
        if constexpr (graph_is_pq(BITS))
            graph_pq_build_tables<METRIC, BITS>(a, reinterpret_cast<float *>(L.qs), reinterpret_cast<const float *>(a.Q + (size_t)q * a.ld4), tid);
        else
        {
            const uint32_t q4 = BITS == 8 ? a.lc4 : a.ld4;
            for (uint32_t i = tid; i < q4; i += BLOCK)
                L.qs[i] = i < a.ld4 ? a.Q[(size_t)q * a.ld4 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        uint4 * clear = reinterpret_cast<uint4 *>(L.table);
        for (uint32_t i = tid; i < a.tab / 4; i += BLOCK)
            clear[i] = make_uint4(GRAPH_EMPTY, GRAPH_EMPTY, GRAPH_EMPTY, GRAPH_EMPTY);
        if (tid < GRAPH_WIDE_CTL)
            L.ctl[tid] = 0;
        __threadfence(); // the clear is in memory before the first atomic asks
        __syncthreads();
        // the seeds of the probed lists
        uint32_t lab = GRAPH_EMPTY;
        if (tid < a.P)
        {
            const int32_t l = a.probes[(size_t)q * a.P + tid];
            const int32_t s = l >= 0 ? a.seed[l] : -1;
            if (s >= 0 && (uint32_t)s < a.n)
                lab = (uint32_t)s;
        }
        graph_wide_round<METRIC, BITS, E>(a, L, flag, lab, tid);
        for (uint32_t it = 0; it < a.max_iters; it++)
        {
            const uint32_t cnt = L.ctl[2];
            if (L.ctl[1] + fan > MSVS_GRAPH_WIDE_VISITED_MAX)
                break;
            // the first `width` clear flags from the cursor on
            uint32_t found = 0;
            for (uint32_t base = L.ctl[4]; found < a.width && base < cnt; base += BLOCK)
            {
                const uint32_t i = base + tid;
                const bool open = i < cnt && flag[i] == 0;
                const uint64_t b = __ballot(open);
                if (lane == 0)
                    ballots[wave] = b;
                __syncthreads();
                uint32_t before = 0, total = 0;
                for (uint32_t w = 0; w < 4; w++)
                {
                    const uint32_t c = (uint32_t)__popcll(ballots[w]);
                    before += w < wave ? c : 0;
                    total += c;
                }
                const uint32_t at = found + before + (uint32_t)__popcll(b & ((1ull << lane) - 1));
                if (open && at < a.width)
                {
                    parents[at] = i;
                    flag[i] = 1;
                    atomicMax(&L.ctl[4], i + 1); // everything up to a parent is expanded now
                }
                found += total;
                __syncthreads(); // (the next window's ballots must not overtake a reader)
            }
            if (found == 0)
                break;
            found = min(found, a.width);
            lab = GRAPH_EMPTY;
            const uint32_t p = tid >> a.lgR;
            if (tid < fan && p < found)
            {
                const uint32_t parent = (uint32_t)L.beam[parents[p]];
                const uint32_t e = a.nbr[(size_t)parent * a.R + (tid & (a.R - 1))];
                lab = e < a.n ? e : GRAPH_EMPTY;
            }
            graph_wide_round<METRIC, BITS, E>(a, L, flag, lab, tid);
        }
        // the first k alive entries of the beam
        const uint32_t cnt = L.ctl[2];
        uint32_t alive = 0;
        for (uint32_t base = 0; base < cnt && alive < a.k; base += BLOCK)
        {
            const uint32_t i = base + tid;
            const uint64_t key = i < cnt ? L.beam[i] : KEY_NONE;
            bool ok = key != KEY_NONE;
            if (ok && a.alive)
            {
                const uint32_t id = (uint32_t)key;
                ok = id < a.nbits && ((a.alive[id >> 6] >> (id & 63)) & 1);
            }
            const uint64_t bo = __ballot(ok);
            if (lane == 0)
                ballots[wave] = bo;
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < 4; w++)
            {
                const uint32_t c = (uint32_t)__popcll(ballots[w]);
                before += w < wave ? c : 0;
                total += c;
            }
            const uint32_t rank = alive + before + (uint32_t)__popcll(bo & ((1ull << lane) - 1));
            if (ok && rank < a.k)
            {
                const size_t o = (size_t)q * a.k + rank;
                a.out_ids[o] = (int64_t)(uint32_t)key;
                const float v = key_value<METRIC>(key);
                a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
            }
            alive += total;
            __syncthreads();
        }
        for (size_t i = (size_t)alive + tid; i < a.k; i += BLOCK)
        {
            const size_t o = (size_t)q * a.k + i;
            a.out_ids[o] = -1;
            const float v = key_value<METRIC>(KEY_NONE);
            a.out_dis[o] = a.cosine ? __fsub_rn(1.0f, v) : v;
        }
    }
}

// ------------------------------------------------------------------------------------------- build

/// ids [n][kk] of an exact search of row i0 + i (labels or -1) -> L[i0 + i][0 .. K0): label i0 + i removed if present, else the last
/// entry dropped; kk = K0 + 1
static __global__ void graph_lists_kernel(const int64_t * ids, uint32_t cnt, uint32_t i0, uint32_t K0, int32_t * L)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt)
        return;
    const int64_t * src = ids + (size_t)i * (K0 + 1);
    int32_t * dst = L + (size_t)(i0 + i) * K0;
    uint32_t o = 0;
    for (uint32_t j = 0; j <= K0 && o < K0; j++)
        if (src[j] != (int64_t)(i0 + i))
            dst[o++] = (int32_t)src[j];
}

// ------------------------------------------------------------------------------------------- build: the join (join_iters >= 1)

// float4 pieces of a row a lane requests ahead of their use.  From the compiler's resource report (gfx950): two sets of 8 take 120
// VGPRs, the search's 4 waves per SIMD, no scratch; two sets of 12 (all of d = 768) take 169 VGPRs, 2 waves.  Not yet timed.
constexpr uint32_t GRAPH_JOIN_HEAD = 8;
constexpr uint32_t GRAPH_JOIN_FETCH = 4; // list words a thread requests before it visits the first of them

struct GraphJoinParams
{
    const float4 * rows;    // n x ld4, zero padded, in HBM
    const float4 * Q;       // the launch's nodes as queries: gridDim.x x ld4, zero padded (normalised again for cosine)
    const int32_t * lists;  // n x K0: L^t, read only
    int32_t * next;         // n x K0: L^{t+1}
    uint32_t * changed;     // += 1 for every node whose list changed
    uint32_t n, i0, ld4, K0, S, cap, tab; // i0: the launch's first node; cap = K0 (S + 1); tab: a power of two >= 2 (cap + 1)
};

inline uint32_t graph_join_table(uint32_t cap)
{
    uint32_t tab = 64;
    while (tab < 2 * (cap + 1))
        tab <<= 1;
    return tab;
}

/// the query | beam, staged keys, flags (256 each) | the score list (cap) | the node's own list (K0) | control words | the visited table
inline size_t graph_join_lds_bytes(uint32_t ld4, uint32_t K0, uint32_t cap, uint32_t tab)
{
    return (size_t)ld4 * 16 + GRAPH_ROUND * (8 + 8 + 4) + ((size_t)cap + K0 + GRAPH_CTL + tab) * 4;
}

/// One join iteration of include/msvs.h's build step 3b, one block of 256 threads per node i:
///   C_i = L_i and the first S entries of the lists of L_i's members, without i and without duplicates; L'_i = its K0 lowest keys.
/// The whole of C_i is known after two dependent loads and nothing in it waits for a merge, so the kernel
///   1. gathers: L_i, then all K0 x S neighbour words, GRAPH_JOIN_FETCH requests a thread at a time; every word goes through the
///      visited table (i sits there from the start) and the winners are compacted into ONE score list;
///   2. scores the list as one stream: group grp takes its labels grp, grp + 16, ... with the NEXT label's first GRAPH_JOIN_HEAD
///      pieces requested before this label's arithmetic (two named register sets, swapped by unrolling), and every 256 labels the
///      staged keys go through graph_merge into a beam of K0 -- the requests of the next chunk's first rows are in flight across
///      the merge and its barriers.  The arithmetic and its order are canonical_row_chain's, so a key is the search's;
///   3. writes the beam's labels (-1 beyond its fill) to the other list buffer and counts the node if its list changed.
template <int METRIC>
static __global__ __launch_bounds__(BLOCK) void graph_join_kernel(const GraphJoinParams a)
{
    extern __shared__ __align__(16) unsigned char graph_lds[];
    GraphLds L;
    L.qs = reinterpret_cast<float4 *>(graph_lds);
    L.vm = L.st = nullptr;
    L.beam = reinterpret_cast<uint64_t *>(graph_lds + (size_t)a.ld4 * 16);
    L.stage = L.beam + GRAPH_ROUND;
    L.flag = reinterpret_cast<uint32_t *>(L.stage + GRAPH_ROUND);
    L.slab = L.flag + GRAPH_ROUND;
    int32_t * mine = reinterpret_cast<int32_t *>(L.slab + a.cap);
    L.ctl = reinterpret_cast<uint32_t *>(mine + a.K0);
    L.table = L.ctl + GRAPH_CTL;
    const uint32_t tid = threadIdx.x, lane = tid & 63, grp = tid >> 4, g = tid & 15, node = a.i0 + blockIdx.x, K0 = a.K0;
    for (uint32_t i = tid; i < a.ld4; i += BLOCK)
        L.qs[i] = a.Q[(size_t)blockIdx.x * a.ld4 + i];
    const uint32_t home = graph_home(node, a.tab);
    for (uint32_t i = tid; i < a.tab; i += BLOCK)
        L.table[i] = i == home ? node : GRAPH_EMPTY; // the node is visited before anybody asks: it is never scored
    if (tid < GRAPH_CTL)
        L.ctl[tid] = 0;
    if (tid < K0)
    {
        const int32_t v = a.lists[(size_t)node * K0 + tid];
        mine[tid] = v >= 0 && (uint32_t)v < a.n ? v : -1;
    }
    __syncthreads();
    // 1. gather and dedup: word e < K0 is L_i[e]; word K0 + x is entry x % S of the list of L_i[x / S]
    for (uint32_t e0 = 0; e0 < a.cap; e0 += BLOCK * GRAPH_JOIN_FETCH)
    {
        uint32_t w[GRAPH_JOIN_FETCH];
#pragma unroll
        for (uint32_t u = 0; u < GRAPH_JOIN_FETCH; u++)
        {
            const uint32_t e = e0 + u * BLOCK + tid;
            w[u] = GRAPH_EMPTY;
            if (e < K0)
                w[u] = (uint32_t)mine[e];
            else if (e < a.cap)
            {
                const uint32_t x = e - K0;
                const int32_t j = mine[x / a.S];
                if (j >= 0)
                {
                    const int32_t v = a.lists[(size_t)j * K0 + x % a.S];
                    w[u] = v >= 0 && (uint32_t)v < a.n ? (uint32_t)v : GRAPH_EMPTY;
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < GRAPH_JOIN_FETCH; u++)
        {
            const bool won = w[u] != GRAPH_EMPTY && graph_visit(L.table, a.tab, w[u]);
            const uint32_t place = graph_wave_place(&L.ctl[0], won, lane);
            if (won)
                L.slab[place] = w[u];
        }
    }
    __syncthreads();
    // 2. score in one stream
    const uint32_t total = L.ctl[0], jfull = a.ld4 >> 4, jtail = a.ld4 & 15;
    const uint32_t np = jfull + (g < jtail ? 1u : 0u), nu = jfull + (jtail ? 1u : 0u); // pieces of this lane; of the longest lane
    auto request = [&](float4(&y)[GRAPH_JOIN_HEAD], const uint32_t id) {
        const float4 * row = a.rows + (size_t)id * a.ld4;
#pragma unroll
        for (uint32_t u = 0; u < GRAPH_JOIN_HEAD; u++)
        {
            y[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (u < nu) // (uniform; a lane without the tail piece asks for the row's first piece again and drops it)
                y[u] = row[u < np ? u * 16 + g : 0];
        }
    };
    auto score = [&](const float4(&y)[GRAPH_JOIN_HEAD], const uint32_t id) {
        const float4 * yrow = a.rows + (size_t)id * a.ld4 + g;
        const float4 * qrow = L.qs + g;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (uint32_t u = 0; u < GRAPH_JOIN_HEAD; u++)
            if (u < np)
                canonical_update<METRIC>(acc, qrow[u * 16], y[u]);
        if (jfull >= GRAPH_JOIN_HEAD) // the rest of a long row, as canonical_row_chain walks it
        {
            uint32_t j = GRAPH_JOIN_HEAD;
            for (; j + 4 <= jfull; j += 4)
            {
                const float4 y0 = yrow[j * 16], y1 = yrow[(j + 1) * 16], y2 = yrow[(j + 2) * 16], y3 = yrow[(j + 3) * 16];
                canonical_update<METRIC>(acc, qrow[j * 16], y0);
                canonical_update<METRIC>(acc, qrow[(j + 1) * 16], y1);
                canonical_update<METRIC>(acc, qrow[(j + 2) * 16], y2);
                canonical_update<METRIC>(acc, qrow[(j + 3) * 16], y3);
            }
            for (; j < jfull; j++)
                canonical_update<METRIC>(acc, qrow[j * 16], yrow[j * 16]);
            if (g < jtail)
                canonical_update<METRIC>(acc, qrow[jfull * 16], yrow[jfull * 16]);
        }
        const float s = row16_tree_sum(__fadd_rn(__fadd_rn(acc.x, acc.y), __fadd_rn(acc.z, acc.w)));
        return make_key<METRIC>(s, id);
    };
    float4 ya[GRAPH_JOIN_HEAD], yb[GRAPH_JOIN_HEAD];
    if (grp < total)
        request(ya, L.slab[grp]);
    for (uint32_t base = 0; base < total; base += GRAPH_ROUND)
    {
        for (uint32_t c = base + grp; c < min(base + GRAPH_ROUND, total); c += 32) // two labels a trip: ya holds label c's head
        {
            const uint32_t ida = L.slab[c], idb = c + 16 < total ? L.slab[c + 16] : GRAPH_EMPTY;
            if (idb != GRAPH_EMPTY)
                request(yb, idb);
            const uint64_t ka = score(ya, ida);
            if (g == 0)
                L.stage[c - base] = ka;
            if (c + 32 < total) // (the trip's last label of a chunk asks for the next chunk's first)
                request(ya, L.slab[c + 32]);
            if (idb != GRAPH_EMPTY)
            {
                const uint64_t kb = score(yb, idb);
                if (g == 0)
                    L.stage[c + 16 - base] = kb;
            }
        }
        __syncthreads();
        graph_merge(L, K0, min(GRAPH_ROUND, total - base), L.ctl[2], tid);
    }
    // 3. the new list
    const uint32_t cnt = L.ctl[2];
    bool differs = false;
    if (tid < K0)
    {
        const int32_t v = tid < cnt ? (int32_t)(uint32_t)L.beam[tid] : -1;
        a.next[(size_t)node * K0 + tid] = v;
        differs = v != mine[tid];
    }
    if (__ballot(differs) && lane == 0)
        L.ctl[4] = 1;
    __syncthreads();
    if (tid == 0 && L.ctl[4])
        atomicAdd(a.changed, 1u);
}

inline size_t graph_prune_lds_bytes(uint32_t K0) { return ((size_t)K0 * K0 + 2 * K0) * 4; }

/// One block per node i: its list and the lists of its K0 neighbours sit in LDS (K0 x K0 x 4 bytes); detour(b) counts the a < b
/// whose list holds L_i[b] at a position r < b; F_i = the valid entries by (detour, b), cut to R.  Integer work only.
static __global__ __launch_bounds__(BLOCK) void graph_prune_kernel(const int32_t * L, uint32_t n, uint32_t K0, uint32_t R, uint32_t * F)
{
    extern __shared__ __align__(16) unsigned char graph_lds[];
    int32_t * mine = reinterpret_cast<int32_t *>(graph_lds);
    uint32_t * detour = reinterpret_cast<uint32_t *>(mine + K0);
    int32_t * lists = mine + 2 * K0; // [a][r]
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    if (tid < K0)
    {
        const int32_t v = L[(size_t)i * K0 + tid];
        mine[tid] = v >= 0 && (uint32_t)v < n ? v : -1;
        detour[tid] = 0;
    }
    if (tid < R)
        F[(size_t)i * R + tid] = GRAPH_EMPTY;
    __syncthreads();
    for (uint32_t e = tid; e < K0 * K0; e += BLOCK)
    {
        const int32_t a = mine[e / K0];
        lists[e] = a >= 0 ? L[(size_t)a * K0 + e % K0] : -1;
    }
    __syncthreads();
    // thread (b, slice): the a of its slice below b
    const uint32_t b = tid % K0, slices = BLOCK / K0, slice = tid / K0; // K0 <= 128: at least two slices
    const int32_t target = mine[b];
    if (slice < slices && target >= 0)
    {
        uint32_t d = 0;
        for (uint32_t a = slice; a < b; a += slices)
        {
            if (mine[a] < 0)
                continue;
            bool hit = false;
            for (uint32_t r = 0; r < b; r++)
                hit |= lists[a * K0 + r] == target;
            d += hit ? 1u : 0u;
        }
        if (d)
            atomicAdd(&detour[b], d);
    }
    __syncthreads();
    if (tid < K0 && mine[tid] >= 0)
    {
        const uint32_t d = detour[tid];
        uint32_t rank = 0;
        for (uint32_t c = 0; c < K0; c++)
            rank += mine[c] >= 0 && (detour[c] < d || (detour[c] == d && c < tid)) ? 1u : 0u;
        if (rank < R)
            F[(size_t)i * R + rank] = (uint32_t)mine[tid];
    }
}

/// incoming edges of every node: cnt[F[i][r]]++
static __global__ void graph_count_kernel(const uint32_t * F, size_t words, uint32_t * cnt)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < words && F[e] != GRAPH_EMPTY)
        atomicAdd(&cnt[F[e]], 1u);
}

/// off[0 .. n] = exclusive prefix sums of cnt[0 .. n) (one block; 64-bit: n x R edges); cnt is cleared for the scatter's fill counters
static __global__ __launch_bounds__(BLOCK) void graph_scan_kernel(uint32_t * cnt, uint32_t n, uint64_t * off)
{
    __shared__ uint64_t part[BLOCK];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0)
        carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += BLOCK)
    {
        const uint32_t i = base + tid;
        const uint64_t v = i < n ? cnt[i] : 0;
        part[tid] = v;
        __syncthreads();
        for (uint32_t s = 1; s < BLOCK; s <<= 1)
        {
            const uint64_t add = tid >= s ? part[tid - s] : 0;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        if (i < n)
        {
            off[i] = carry + part[tid] - v;
            cnt[i] = 0;
        }
        __syncthreads();
        if (tid == BLOCK - 1)
            carry += part[tid];
        __syncthreads();
    }
    if (tid == 0)
        off[n] = carry;
}

/// edge (r, i) with F[i][r] = j goes somewhere into j's segment: the place is the atomics' business, the selection ranks the keys
static __global__ void graph_scatter_kernel(const uint32_t * F, size_t words, uint32_t lgR, const uint64_t * off, uint32_t * fill, uint64_t * seg)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= words || F[e] == GRAPH_EMPTY)
        return;
    const uint32_t j = F[e], i = (uint32_t)(e >> lgR), r = (uint32_t)e & ((1u << lgR) - 1);
    seg[off[j] + atomicAdd(&fill[j], 1u)] = (uint64_t)r << 32 | i;
}

/// One wavefront per node j: G_j = the sources of the R / 2 smallest (r, i) of its segment (R / 2 passes of "the smallest key above
/// the last one"), then N_j = F_j[0 .. R/2), the G_j not yet there, the F_j[R/2 .. R) not yet there, compacted and cut to R.
static __global__ __launch_bounds__(BLOCK) void graph_reverse_kernel(const uint32_t * F, const uint64_t * off, const uint64_t * seg, uint32_t n,
                                                                     uint32_t R, uint32_t * nbr)
{
    __shared__ uint32_t cand_all[4][96]; // R / 2 + R / 2 + R / 2 <= 96 candidates of a node, in order
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, H = R / 2;
    const bool live = blockIdx.x * 4 + wave < n; // (the last block's spare wavefronts keep the barriers company on node 0, and write nothing)
    const uint32_t j = live ? blockIdx.x * 4 + wave : 0;
    uint32_t * cand = cand_all[wave];
    for (uint32_t s = lane; s < 3 * H; s += 64)
        cand[s] = s < H ? F[(size_t)j * R + s] : (s < 2 * H ? GRAPH_EMPTY : F[(size_t)j * R + s - H]);
    __syncthreads();
    const uint64_t s0 = off[j], s1 = off[j + 1];
    uint64_t last = 0;
    for (uint32_t t = 0; t < H && s0 + t < s1; t++)
    {
        uint64_t best = KEY_NONE;
        for (uint64_t e = s0 + lane; e < s1; e += 64)
        {
            const uint64_t key = seg[e];
            if ((t == 0 || key > last) && key < best)
                best = key;
        }
        for (int d = 32; d; d >>= 1)
        {
            const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)best, d);
            best = o < best ? o : best;
        }
        last = best;
        if (lane == 0)
            cand[H + t] = (uint32_t)best;
    }
    __syncthreads();
    uint32_t placed = 0;
    for (uint32_t s = lane; s < ((3 * H + 63) & ~63u); s += 64) // whole wavefronts: every lane votes
    {
        const uint32_t v = s < 3 * H ? cand[s] : GRAPH_EMPTY;
        bool keep = v != GRAPH_EMPTY;
        for (uint32_t e = 0; keep && e < s; e++)
            keep = cand[e] != v;
        const uint64_t b = __ballot(keep);
        const uint32_t at = placed + (uint32_t)__popcll(b & ((1ull << lane) - 1));
        if (live && keep && at < R)
            nbr[(size_t)j * R + at] = v;
        placed += (uint32_t)__popcll(b);
    }
    for (uint32_t s = placed + lane; live && s < R; s += 64)
        nbr[(size_t)j * R + s] = GRAPH_EMPTY;
}

}
