// graph_index.hip -- the graph index (include/msvs.h: msvs_graph_index_*): coarse centroids, one seed label per centroid and a
// fixed-degree neighbour graph over the rows of a borrowed row store; searched by a seeded beam search whose every id and distance
// is a function of the inputs alone.  The kernels and their layout: graph_kernels.hpp.  DESIGN.md 4.14.
// bit_size=8: the index keeps one 8-bit quantiser and a code row per label, made from the store by build / set_graph; the search
// scores decoded rows and nothing but build / set_graph reads the store.
// bit_size=16: the index keeps one binary16 row per label (graph_h16_encode_kernel, graph_h16_slot's order), no quantiser; the search
// scores the exactly decoded rows with the f32 search's LDS image; file version 4.
// pq_m=M: the index keeps M sub-codebooks (trained over the store by the IVFPQ index's codebook step, or handed in) and M codes a
// label in GraphPqLayout's order; the search scores a label by M look-ups into a per-query table; file version 3.
// search_wide: the same definition with ef, k <= MSVS_MAX_K_ROUNDS, served by graph_wide_search_kernel on a fixed grid.
// Reused as they are: the row store (refine.hip), the canonical scoring of refine_kernels.hpp's chain, the k-means trainer and the
// canonical coarse top-P (coded_ivf.hpp: kmeans, flat_search_device), the exact FLAT search for the build's neighbour lists -- or,
// with join_iters >= 1, an IVFFLAT search of build_nprobe lists whose lists graph_join_kernel repairs across partition borders.
#include <algorithm>
#include <cmath>
#include <memory>
#include <mutex>

#include "coded_ivf.hpp"
#include "graph_kernels.hpp"

using namespace msvs;

static_assert(MSVS_MAX_K <= GRAPH_ROUND, "a beam entry, a seed and a staged key per thread of a block");

struct msvs_graph_index
{
    int metric = MSVS_METRIC_L2;
    size_t dim = 0, n = 0, nlist = 0;
    uint32_t ld = 0, R = 32;
    // the build (create's join_iters, build_nprobe, join_sample): 0 iterations is the exact O(n^2) build
    size_t join_iters = 0, build_nprobe = 8;
    uint32_t join_sample = 8;
    int device = 0;
    std::string params;
    const msvs_rows * rows = nullptr; // borrowed
    DevBuf<float> centroids;          // nlist x ld
    DevBuf<int32_t> seeds;            // nlist
    DevBuf<uint32_t> nbr;             // n x R
    // bit_size=8 (ldc = round_up(dim, 16) bytes a stored row, sq_layout.hpp's 8-bit order; ldc floats of padded vmin / step)
    uint32_t bits = 32, ldc = 0;
    std::vector<float> h_vmin, h_vmax; // dim
    DevBuf<float> d_vmin, d_step;      // ldc, zero padded
    DevBuf<uint8_t> codes;             // n x ldc
    // bit_size=16: codes holds n x ldc binary16 values in graph_h16_slot's order; no quantiser
    // pq_m=M (bits is then the width of a code, 8 or 4; no quantiser, ldc unused): codes holds n rows of GraphPqLayout
    size_t pq_m = 0;
    bool cb_handed = false;  // h_cb came through set_pq_codebooks: build / set_graph encode only
    std::vector<float> h_cb; // [m][ksub][dsub]
    DevBuf<float> cbT;       // the same in pq_cb_index's order
    bool ready = false;
    bool sq() const { return bits == 8 && !pq_m; }
    bool h16() const { return bits == 16 && !pq_m; }
    bool coded() const { return bits != 32 || pq_m; } // the search reads the index's own rows, never the store
    size_t ksub() const { return (size_t)1 << bits; }
    GraphPqLayout pq_layout() const { return GraphPqLayout((uint32_t)pq_m, bits); }
};

namespace
{
const char * const GRAPH = "graph";
constexpr size_t GRAPH_LDS_MAX = 160 * 1024;
constexpr size_t GRAPH_QUERY_CHUNK = 16384; // queries of one coarse step + launch
constexpr size_t GRAPH_LIST_CHUNK = 4096;   // rows whose exact lists one FLAT search of the build returns
constexpr size_t GRAPH_CODE_CHUNK = (size_t)1 << 27; // codes one launch of the encoder writes
constexpr size_t GRAPH_PQ_TRAIN_ROWS = 262144;       // stored rows the sub-codebooks are trained on at most (the IVFPQ index's number)

uint32_t log2_of(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v)
        l++;
    return l;
}

void check_graph(const msvs_graph_index * ix)
{
    if (!ix)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
}

void check_graph_ready(const msvs_graph_index & ix)
{
    if (!ix.ready)
        fail(MSVS_ERR_NOT_READY, "the graph index has no graph yet (build / set_graph)");
}

struct GraphSearch // the search parameters, defaults filled in
{
    size_t ef = 0, nprobe = 8, width = 1, max_iters = 0;
};

/// ef 0: max(k, 64) capped at ef_max (MSVS_MAX_K; the wide search: MSVS_MAX_K_ROUNDS); max_iters 0: ceil(2 ef / width) + 8
GraphSearch graph_defaults(size_t k, size_t ef, size_t nprobe, size_t width, size_t max_iters, size_t ef_max)
{
    GraphSearch s;
    s.ef = ef ? ef : std::min<size_t>(std::max<size_t>(k, 64), ef_max);
    s.nprobe = nprobe;
    s.width = width;
    if (s.ef > ef_max || width < 1 || width > 4 || nprobe < 1)
        fail(MSVS_ERR_INVALID_ARGUMENT, "graph search needs 1 <= ef <= %zu, 1 <= width <= 4 and nprobe >= 1 (ef %zu, width %zu, nprobe %zu)", ef_max,
             s.ef, width, nprobe);
    s.max_iters = max_iters ? max_iters : ceil_div(2 * s.ef, width) + 8;
    return s;
}

GraphSearch parse_graph_search(const char * params, size_t k, size_t ef_max)
{
    const auto p = parse_params(params);
    for (const auto & kv : p)
        if (kv.first != "ef" && kv.first != "nprobe" && kv.first != "width" && kv.first != "max_iters")
            fail(MSVS_ERR_INVALID_ARGUMENT, "unknown search parameter `%s`", kv.first.c_str());
    const long ef = param_int(p, "ef", 0), nprobe = param_int(p, "nprobe", 8), width = param_int(p, "width", 1), it = param_int(p, "max_iters", 0);
    if ((p.count("ef") && ef < 1) || nprobe < 1 || width < 1 || (p.count("max_iters") && it < 1))
        fail(MSVS_ERR_INVALID_ARGUMENT, "ef, nprobe, width and max_iters must be >= 1");
    return graph_defaults(k, (size_t)ef, (size_t)nprobe, (size_t)width, (size_t)it, ef_max);
}

template <int METRIC, int BITS>
void launch_graph_search(const GraphSearchParams & a, size_t nq, size_t lds, hipStream_t stream)
{
    constexpr auto kernel = &graph_search_kernel<METRIC, BITS>;
    static std::once_flag once; // more than 64 KiB of dynamic LDS needs the attribute raised once per kernel
    std::call_once(once, [] {
        MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRAPH_LDS_MAX));
    });
    hipLaunchKernelGGL(kernel, dim3((unsigned)nq), dim3(BLOCK), lds, stream, a);
}

// The wide search's grid is fixed: as many blocks as stay resident, each with a visited table of its own in the stream's arena.
constexpr size_t GRAPH_WIDE_TABLE_BUDGET = (size_t)1 << 30; // bytes of visited tables of one launch at most
constexpr size_t GRAPH_WIDE_CU_LDS = 160 * 1024;            // blocks per CU: the LDS images that fit a CU's 160 KiB ...
constexpr size_t GRAPH_WIDE_CU_BLOCKS = 4;                  // ... and at most 4: a block is a wavefront per SIMD, the kernel takes 113 .. 150 VGPRs

/// the beam entries a thread of the wide kernel holds: the kernel's E for this ef
int graph_wide_entries(size_t ef)
{
    int e = 1;
    while ((size_t)e * BLOCK < ef)
        e *= 2;
    return e;
}

template <int METRIC, int BITS, int E>
void launch_graph_wide_search(const GraphWideParams & a, unsigned grid, size_t lds, hipStream_t stream)
{
    constexpr auto kernel = &graph_wide_search_kernel<METRIC, BITS, E>;
    static std::once_flag once;
    std::call_once(once, [] {
        MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRAPH_LDS_MAX));
    });
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, stream, a);
}

template <int METRIC>
void launch_graph_join(const GraphJoinParams & a, size_t nodes, size_t lds, hipStream_t stream)
{
    constexpr auto kernel = &graph_join_kernel<METRIC>;
    static std::once_flag once;
    std::call_once(once, [] {
        MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)GRAPH_LDS_MAX));
    });
    hipLaunchKernelGGL(kernel, dim3((unsigned)nodes), dim3(BLOCK), lds, stream, a);
}

/// Everything on the device, enqueued on `stream`: queries padded (normalised for cosine), the canonical coarse top-P, one launch a
/// chunk of queries -- of graph_search_kernel (a block a query, the visited table in LDS), or with `wide` of graph_wide_search_kernel
/// (a fixed grid, the visited tables in the stream's arena).
void graph_search_chunks(const msvs_graph_index & ix, const float * d_queries, size_t nq, size_t k, const GraphSearch & s, const uint64_t * d_alive,
                         size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream, bool wide)
{
    check_k(k, wide ? MSVS_MAX_K_ROUNDS : MSVS_MAX_K);
    check_graph_ready(ix);
    if (k > s.ef)
        fail(MSVS_ERR_UNSUPPORTED_K, "k = %zu exceeds ef = %zu, the beam of the graph search", k, s.ef);
    const size_t P = std::min(s.nprobe, ix.nlist), fan = s.width * ix.R;
    if (P > MSVS_MAX_K)
        fail(MSVS_ERR_UNSUPPORTED_K, "min(nprobe, nlist) = %zu exceeds the coarse quantiser's top-k limit %d", P, MSVS_MAX_K);
    // the visited table: what the search can score at most, at load factor <= 0.5
    const size_t cap = wide ? MSVS_GRAPH_WIDE_VISITED_MAX : MSVS_GRAPH_VISITED_MAX;
    const size_t iters = std::min<size_t>(s.max_iters, cap), reach = std::min<size_t>(cap, P + iters * fan);
    // (the wide kernel clears its table with 16-byte stores: a multiple of four words)
    const uint32_t tab = (uint32_t)round_up(2 * std::max<size_t>(reach, 32), (size_t)(wide ? 4 : 1)), ld4 = ix.ld / 4, lc4 = ix.ldc / 4;
    const bool coded = ix.coded();
    // the float4 before the beam: the query, or query | vmin | step, or the product-quantised tables
    const uint32_t head4 = ix.pq_m ? (uint32_t)(ix.pq_m * ix.ksub() / 4) : ix.sq() ? 3 * lc4 : ld4;
    const size_t lds = wide ? graph_wide_lds_bytes(head4, (uint32_t)s.ef) : graph_lds_bytes(head4, tab);
    if (lds > GRAPH_LDS_MAX)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the graph search's LDS image (%zu bytes) exceeds %zu", lds, GRAPH_LDS_MAX);
    if (nq == 0 || k == 0)
        return;
    if (!d_queries || !d_ids || !d_dis)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    const float * table = nullptr; // (a coded index never looks at the store)
    if (!coded)
    {
        const RowsView rv = rows_view(ix.rows);
        if (rv.n < ix.n)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the row store holds %zu rows, the graph was made over %zu", rv.n, ix.n);
        table = rv.table;
    }
    const int m = scan_metric(ix.metric);
    const size_t chunk = std::min(nq, GRAPH_QUERY_CHUNK);
    // the wide grid: the blocks the device keeps resident, no more than there are queries or tables within the budget
    const size_t per_cu = std::max<size_t>(1, std::min(GRAPH_WIDE_CU_LDS / lds, GRAPH_WIDE_CU_BLOCKS));
    const size_t grid = wide ? std::max<size_t>(1, std::min({chunk, per_cu * device_cu_count(), GRAPH_WIDE_TABLE_BUDGET / ((size_t)tab * 4)})) : 0;
    Scratch & scr = scratch_for(stream);
    scr.reserve(chunk * ((size_t)ix.ld * 4 + P * 4) + flat_scratch_bytes(ix.nlist, chunk, (uint32_t)P, ix.ld) + grid * tab * 4 + 9 * 256, stream);
    float * dq = scr.take<float>(chunk * ix.ld);
    int32_t * probes = scr.take<int32_t>(chunk * P);
    uint32_t * tables = wide ? scr.take<uint32_t>(grid * tab) : nullptr;
    const size_t mark = scr.used;
    for (size_t q0 = 0; q0 < nq; q0 += chunk)
    {
        const size_t nqc = std::min(chunk, nq - q0);
        upload_rows(dq, d_queries + q0 * ix.dim, nqc, (uint32_t)ix.dim, ix.ld, MSVS_MEM_DEVICE, stream);
        if (ix.metric == MSVS_METRIC_COSINE)
            normalize_device_rows(dq, nqc, (uint32_t)ix.dim, ix.ld, stream);
        scr.used = mark;
        MergeParams co{};
        co.mode = 1;
        co.out_probes = probes;
        flat_search_device(scr, m, ix.centroids.p, nullptr, ix.nlist, ix.ld, dq, nqc, (uint32_t)P, nullptr, 0, co, stream);
        GraphWideParams a{};
        a.tables = tables;
        a.nq = (uint32_t)nqc;
        a.rows = reinterpret_cast<const float4 *>(table);
        a.codes = reinterpret_cast<const uint4 *>(ix.codes.p);
        a.vmin = reinterpret_cast<const float4 *>(ix.d_vmin.p);
        a.step = reinterpret_cast<const float4 *>(ix.d_step.p);
        a.lc4 = lc4;
        if (ix.pq_m)
        {
            const GraphPqLayout lay = ix.pq_layout();
            a.pq_cb = ix.cbT.p;
            a.pq_m = lay.m;
            a.pq_dsub = (uint32_t)(ix.dim / ix.pq_m);
            a.pq_c = lay.c;
            a.pq_w = lay.w;
        }
        a.Q =reinterpret_cast<const float4 *>(dq);
        a.nbr = ix.nbr.p;
        a.seed = ix.seeds.p;
        a.probes = probes;
        a.alive = d_alive;
        a.out_ids = d_ids + q0 * k;
        a.out_dis = d_dis + q0 * k;
        a.nbits = (uint32_t)std::min<size_t>(nbits, 0xffffffffu);
        a.n = (uint32_t)ix.n;
        a.ld4 = ld4;
        a.R = ix.R;
        a.lgR = log2_of(ix.R);
        a.ef = (uint32_t)s.ef;
        a.k = (uint32_t)k;
        a.width = (uint32_t)s.width;
        a.max_iters = (uint32_t)std::min<size_t>(s.max_iters, 0xffffffffu);
        a.P = (uint32_t)P;
        a.tab = tab;
        a.cosine = ix.metric == MSVS_METRIC_COSINE;
        ProfileScope prof(wide ? "graph_wide_search" : "graph_search", stream);
        with_int<M_IP, M_L2>(m, [&](auto mm) {
            with_int<8, 32, 16, GRAPH_PQ8, GRAPH_PQ4>(ix.pq_m ? (ix.bits == 8 ? GRAPH_PQ8 : GRAPH_PQ4) : (int)ix.bits, [&](auto bb) {
                constexpr int METRIC = decltype(mm)::value, BITS = decltype(bb)::value;
                if (!wide)
                    launch_graph_search<METRIC, BITS>(a, nqc, lds, stream);
                else
                    with_int<1, 2, 4, 8, 16>(graph_wide_entries(s.ef), [&](auto ee) {
                        launch_graph_wide_search<METRIC, BITS, decltype(ee)::value>(a, (unsigned)std::min(grid, nqc), lds, stream);
                    });
            });
        });
        MSVS_HIP(hipGetLastError());
    }
}

void graph_search_device(const msvs_graph_index & ix, const float * d_queries, size_t nq, size_t k, const GraphSearch & s, const uint64_t * d_alive,
                         size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    graph_search_chunks(ix, d_queries, nq, k, s, d_alive, nbits, d_ids, d_dis, stream, false);
}

/// the wide search (include/msvs.h): ef and k up to MSVS_MAX_K_ROUNDS, always graph_wide_search_kernel
void graph_wide_search_device(const msvs_graph_index & ix, const float * d_queries, size_t nq, size_t k, const GraphSearch & s,
                              const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    graph_search_chunks(ix, d_queries, nq, k, s, d_alive, nbits, d_ids, d_dis, stream, true);
}

/// centroids (nlist x dim, host), seeds and edges (host) -> the index's device buffers; the caller has validated them
void install_graph(msvs_graph_index & ix, const float * centroids, size_t nlist, const int32_t * seeds, const uint32_t * nbr, hipStream_t stream)
{
    ix.nlist = nlist;
    ix.centroids.alloc(nlist * ix.ld);
    upload_rows(ix.centroids.p, centroids, nlist, (uint32_t)ix.dim, ix.ld, MSVS_MEM_HOST, stream);
    ix.seeds.alloc(nlist);
    MSVS_HIP(hipMemcpyAsync(ix.seeds.p, seeds, nlist * 4, hipMemcpyHostToDevice, stream));
    ix.nbr.alloc(std::max<size_t>(ix.n * ix.R, 1));
    if (ix.n)
        MSVS_HIP(hipMemcpyAsync(ix.nbr.p, nbr, ix.n * ix.R * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
}

/// bounds (usable: finite, vmax >= vmin, a finite span) -> the index's quantiser: step = fl(fl(vmax - vmin) / 255), both padded with 0
void set_graph_quantiser(msvs_graph_index & ix, const float * vmin, const float * vmax, hipStream_t stream)
{
    ix.h_vmin.assign(vmin, vmin + ix.dim);
    ix.h_vmax.assign(vmax, vmax + ix.dim);
    std::vector<float> pm(ix.ldc, 0.f), ps(ix.ldc, 0.f);
    for (size_t j = 0; j < ix.dim; j++)
    {
        const float range = vmax[j] - vmin[j];
        pm[j] = vmin[j];
        ps[j] = range / 255.0f;
    }
    ix.d_vmin.alloc(ix.ldc);
    ix.d_step.alloc(ix.ldc);
    MSVS_HIP(hipMemcpyAsync(ix.d_vmin.p, pm.data(), ix.ldc * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipMemcpyAsync(ix.d_step.p, ps.data(), ix.ldc * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
}

/// the first dimension whose bounds give no finite step (the rule of the IVFSQ index's sq_unusable_dimension), or dim
size_t graph_unusable_dimension(const float * vmin, const float * vmax, size_t dim)
{
    for (size_t j = 0; j < dim; j++)
        if (!std::isfinite(vmin[j]) || !std::isfinite(vmax[j]) || !std::isfinite(vmax[j] - vmin[j]))
            return j;
    return dim;
}

/// bit_size=8, after build / set_graph (ix.n is set): the quantiser over the store's n rows, then their codes.  The rows are read
/// where they are (HBM or mapped pinned host memory), in chunks, by the IVFSQ index's range and encode kernels against ONE all-zero
/// centroid: fl(x - 0) = x for every x, so the residual is the row and the codes are include/msvs.h's.
void encode_store(msvs_graph_index & ix, hipStream_t stream)
{
    const RowsView rv = rows_view(ix.rows);
    const size_t n = ix.n, dim = ix.dim;
    if (rv.n < n)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the row store holds %zu rows, the graph was made over %zu", rv.n, n);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(n, 1), GRAPH_CODE_CHUNK / ix.ldc));
    DevBuf<float> zero(rv.ld);
    DevBuf<int32_t> list(chunk);
    DevBuf<uint32_t> range(2 * dim);
    MSVS_HIP(hipMemsetAsync(zero.p, 0, (size_t)rv.ld * 4, stream));
    MSVS_HIP(hipMemsetAsync(list.p, 0, chunk * 4, stream));
    MSVS_HIP(hipMemsetAsync(range.p, 0xff, dim * 4, stream));
    MSVS_HIP(hipMemsetAsync(range.p + dim, 0, dim * 4, stream));
    const uint32_t rpb = 64;
    for (size_t r0 = 0; r0 < n; r0 += chunk)
    {
        const size_t m = std::min(chunk, n - r0);
        hipLaunchKernelGGL(sq_range_kernel, dim3((unsigned)ceil_div(m, (size_t)rpb)), dim3(BLOCK), 0, stream, rv.table + r0 * rv.ld, list.p, zero.p, m,
                           (uint32_t)dim, rv.ld, rpb, range.p, range.p + dim);
        MSVS_HIP(hipGetLastError());
    }
    std::vector<uint32_t> ord(2 * dim);
    MSVS_HIP(hipMemcpyAsync(ord.data(), range.p, ord.size() * 4, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    std::vector<float> lo(dim), hi(dim);
    auto value = [](uint32_t o) { // the ordered word of scan_kernels.hpp's f2ord, undone
        const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
        float f;
        memcpy(&f, &u, 4);
        return f;
    };
    for (size_t j = 0; j < dim; j++)
    {
        const bool seen = ord[j] <= ord[dim + j]; // (a column of NaNs, or no row at all: the empty range 0 .. 0)
        lo[j] = seen ? value(ord[j]) : 0.f;
        hi[j] = seen ? value(ord[dim + j]) : 0.f;
    }
    const size_t bad = graph_unusable_dimension(lo.data(), hi.data(), dim);
    if (bad < dim)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the stored rows of dimension %zu span %g .. %g: no finite quantiser step (an infinite row?)", bad,
             (double)lo[bad], (double)hi[bad]);
    set_graph_quantiser(ix, lo.data(), hi.data(), stream);
    ix.codes.alloc(std::max<size_t>(n * ix.ldc, 1));
    for (size_t r0 = 0; r0 < n; r0 += chunk)
    {
        const size_t m = std::min(chunk, n - r0);
        hipLaunchKernelGGL(sq_encode_kernel<8>, dim3((unsigned)ceil_div(m * ix.ldc, (size_t)BLOCK)), dim3(BLOCK), 0, stream, rv.table + r0 * rv.ld, list.p,
                           zero.p, ix.d_vmin.p, ix.d_step.p, m, (uint32_t)dim, rv.ld, ix.ldc, ix.codes.p + r0 * ix.ldc);
        MSVS_HIP(hipGetLastError());
    }
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
}

/// the codes of the index, n x dim in natural column order (export, the file)
std::vector<uint8_t> host_codes(const msvs_graph_index & ix, hipStream_t stream)
{
    std::vector<uint8_t> stored(ix.n * ix.ldc), out(ix.n * ix.dim);
    if (!stored.empty())
        MSVS_HIP(hipMemcpyAsync(stored.data(), ix.codes.p, stored.size(), hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    for (size_t r = 0; r < ix.n; r++)
        for (size_t j = 0; j < ix.dim; j++)
            out[r * ix.dim + j] = stored[r * ix.ldc + sq_stored_pos((uint32_t)j, ix.ldc)];
    return out;
}

/// bit_size=16, after build / set_graph (ix.n is set): the store's n rows as binary16 in the search's stored order.  The rows are
/// read where they are (HBM or mapped pinned host memory), GRAPH_CODE_CHUNK halves a launch.
void encode_h16_store(msvs_graph_index & ix, hipStream_t stream)
{
    const RowsView rv = rows_view(ix.rows);
    const size_t n = ix.n, lc4 = ix.ldc / 4;
    if (rv.n < n)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the row store holds %zu rows, the graph was made over %zu", rv.n, n);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(n, 1), GRAPH_CODE_CHUNK / ix.ldc));
    ix.codes.alloc(std::max<size_t>(n * ix.ldc * 2, 1));
    for (size_t r0 = 0; r0 < n; r0 += chunk)
    {
        const size_t m = std::min(chunk, n - r0);
        hipLaunchKernelGGL(graph_h16_encode_kernel, dim3((unsigned)ceil_div(m * lc4, (size_t)BLOCK)), dim3(BLOCK), 0, stream,
                           reinterpret_cast<const float4 *>(rv.table + r0 * rv.ld), m, rv.ld / 4, (uint32_t)lc4,
                           reinterpret_cast<uint2 *>(ix.codes.p) + r0 * lc4);
        MSVS_HIP(hipGetLastError());
    }
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
}

/// half j of a binary16 stored row of ldc halves
inline size_t h16_stored_pos(size_t j, uint32_t ldc) { return 4 * (size_t)graph_h16_slot((uint32_t)(j / 4), ldc / 4) + j % 4; }

/// the binary16 rows of the index, n x dim in natural column order (the file)
std::vector<uint16_t> host_h16_rows(const msvs_graph_index & ix, hipStream_t stream)
{
    std::vector<uint16_t> stored(ix.n * ix.ldc), out(ix.n * ix.dim);
    if (!stored.empty())
        MSVS_HIP(hipMemcpyAsync(stored.data(), ix.codes.p, stored.size() * 2, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    for (size_t r = 0; r < ix.n; r++)
        for (size_t j = 0; j < ix.dim; j++)
            out[r * ix.dim + j] = stored[r * ix.ldc + h16_stored_pos(j, ix.ldc)];
    return out;
}

void check_graph_coded(const msvs_graph_index & ix)
{
    if (!ix.sq())
        fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index keeps %s: it has no quantiser bounds and scalar codes",
             ix.pq_m     ? "product-quantised codes (pq_m)"
             : ix.h16() ? "binary16 rows (bit_size=16)"
                         : "f32 rows of its row store (bit_size=32)");
}

void check_graph_pq(const msvs_graph_index & ix)
{
    if (!ix.pq_m)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index was created without pq_m: it has no product-quantised form");
}

// ------------------------------------------------------------------------------------------- product-quantised rows (pq_m)

/// codebooks [m][ksub][dsub] on the host, all finite -> the index's host and device copies (pq_cb_index's order); synchronises
void set_graph_codebooks(msvs_graph_index & ix, const float * cb, hipStream_t stream)
{
    const size_t m = ix.pq_m, ksub = ix.ksub(), dsub = ix.dim / m;
    ix.h_cb.assign(cb, cb + ksub * ix.dim);
    std::vector<float> t(ksub * ix.dim);
    with_int<8, 4>((int)ix.bits, [&](auto b) {
        for (uint32_t s = 0; s < m; s++)
            for (uint32_t j = 0; j < ksub; j++)
                for (uint32_t u = 0; u < dsub; u++)
                    t[pq_cb_index<decltype(b)::value>(s, u, j, (uint32_t)m, (uint32_t)dsub)] = cb[((size_t)s * ksub + j) * dsub + u];
    });
    ix.cbT.alloc(t.size());
    MSVS_HIP(hipMemcpyAsync(ix.cbT.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
}

/// the index of the first non-finite float of cb[0 .. count), or count
size_t first_non_finite(const float * cb, size_t count)
{
    for (size_t i = 0; i < count; i++)
        if (!std::isfinite(cb[i]))
            return i;
    return count;
}

/// The IVFPQ index's codebook step over the stored rows themselves (include/msvs.h): the evenly spaced rows floor(i n / cap),
/// then per sub-space the IVFFLAT k-means with create's kmeans_iters and seed.  The sample keeps the store's leading dimension
/// (pq_pick_rows_kernel copies whole padded rows), so a sub-space is a strided view of it.
void train_graph_codebooks(msvs_graph_index & ix, const RowsView & rv, hipStream_t stream)
{
    const size_t n = ix.n, m = ix.pq_m, ksub = ix.ksub(), dsub = ix.dim / m, ld = rv.ld;
    if (n < ksub)
        fail(MSVS_ERR_INVALID_ARGUMENT, "pq_m with bit_size=%u needs at least %zu stored rows to train on (%zu)", ix.bits, ksub, n);
    const size_t cap = std::min(n, GRAPH_PQ_TRAIN_ROWS);
    DevBuf<float> sample(cap * ld), sub(cap * dsub);
    hipLaunchKernelGGL(pq_pick_rows_kernel, dim3((unsigned)ceil_div(cap * ld, (size_t)256)), dim3(256), 0, stream, rv.table, n, cap, (size_t)0, cap,
                       (uint32_t)ld, sample.p);
    MSVS_HIP(hipGetLastError());
    std::string sub_params;
    for (const auto & kv : parse_params(ix.params.c_str()))
        if (kv.first == "kmeans_iters" || kv.first == "seed")
            sub_params += kv.first + "=" + kv.second + ",";
    sub_params += "ncentroids=" + std::to_string(ksub);
    std::vector<float> cb(ksub * ix.dim);
    for (size_t s = 0; s < m; s++)
    {
        MSVS_HIP(hipMemcpy2DAsync(sub.p, dsub * 4, sample.p + s * dsub, ld * 4, dsub * 4, cap, hipMemcpyDeviceToDevice, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        const TmpIndex tmp = kmeans(MSVS_METRIC_L2, dsub, sub_params, sub.p, cap, MSVS_MEM_DEVICE);
        if (tmp->nlist != ksub)
            fail(MSVS_ERR_DEVICE, "internal: sub-quantiser %zu came out with %zu centroids", s, tmp->nlist);
        MSVS_HIP(hipMemcpy2D(cb.data() + s * ksub * dsub, dsub * 4, tmp->centroids.p, (size_t)tmp->ld * 4, dsub * 4, ksub, hipMemcpyDeviceToHost));
    }
    const size_t bad = first_non_finite(cb.data(), cb.size());
    if (bad < cb.size())
        fail(MSVS_ERR_INVALID_ARGUMENT, "codebook entry %zu of sub-quantiser %zu came out not finite: a stored row is NaN, infinite or overflows",
             (bad / dsub) % ksub, bad / (ksub * dsub));
    set_graph_codebooks(ix, cb.data(), stream);
}

/// pq_m, after build / set_graph (ix.n is set): the codebooks unless they were handed in, then the codes.  As encode_store, the
/// rows are read where they are by the IVFPQ index's encoders against ONE all-zero centroid -- fl(0 + cb) = cb in value, so the
/// sub-score is the row's against the entry itself -- a chunk at a time, and graph_pq_repack_kernel puts each chunk into the
/// search's stored order.
void encode_pq_store(msvs_graph_index & ix, hipStream_t stream)
{
    const RowsView rv = rows_view(ix.rows);
    const size_t n = ix.n, m = ix.pq_m, dsub = ix.dim / m;
    if (rv.n < n)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the row store holds %zu rows, the graph was made over %zu", rv.n, n);
    if (!ix.cb_handed)
        train_graph_codebooks(ix, rv, stream);
    const GraphPqLayout lay = ix.pq_layout();
    const uint32_t mp = (uint32_t)ceil_div(m * ix.bits, (size_t)8);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(std::max<size_t>(n, 1), GRAPH_CODE_CHUNK / mp));
    DevBuf<float> zero(rv.ld);
    DevBuf<int32_t> list(chunk);
    DevBuf<uint8_t> natural(chunk * mp);
    MSVS_HIP(hipMemsetAsync(zero.p, 0, (size_t)rv.ld * 4, stream));
    MSVS_HIP(hipMemsetAsync(list.p, 0, chunk * 4, stream));
    ix.codes.alloc(std::max<size_t>(n * lay.row_bytes(), 1));
    static std::once_flag once; // the 8-bit encoder stages a row and its centroid: 64 KiB at dim = 8192, beside its static bytes
    std::call_once(once, [] {
        MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 8192 * 4));
    });
    for (size_t r0 = 0; r0 < n; r0 += chunk)
    {
        const size_t cnt = std::min(chunk, n - r0);
        const float * x = rv.table + r0 * rv.ld;
        if (ix.bits == 4)
            hipLaunchKernelGGL(pq4_encode_kernel, dim3((unsigned)ceil_div(cnt, (size_t)16)), dim3(BLOCK), 0, stream, x, list.p, zero.p, ix.cbT.p, cnt,
                               rv.ld, (uint32_t)m, (uint32_t)dsub, mp, natural.p);
        else
            hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)ceil_div(cnt, (size_t)8)), dim3(BLOCK), 2 * ix.dim * 4, stream, x, list.p, zero.p,
                               ix.cbT.p, cnt, (uint32_t)ix.dim, rv.ld, (uint32_t)m, (uint32_t)dsub, mp, 8u, natural.p);
        hipLaunchKernelGGL(graph_pq_repack_kernel, dim3((unsigned)ceil_div(cnt * lay.row_bytes(), (size_t)256)), dim3(256), 0, stream, natural.p, cnt,
                           lay.m, lay.bits, mp, ix.codes.p + r0 * lay.row_bytes());
        MSVS_HIP(hipGetLastError());
    }
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
}

/// stored rows (GraphPqLayout) <-> n x m codes, a code a byte in natural order
void pq_unpack_rows(const GraphPqLayout & lay, const uint8_t * stored, size_t n, uint8_t * out)
{
    for (size_t r = 0; r < n; r++)
        for (uint32_t s = 0; s < lay.m; s++)
            out[r * lay.m + s] = (uint8_t)((stored[r * lay.row_bytes() + lay.pos(s)] >> lay.shift(s)) & ((1u << lay.bits) - 1));
}

void pq_pack_rows(const GraphPqLayout & lay, const uint8_t * codes, size_t n, uint8_t * stored)
{
    for (size_t r = 0; r < n; r++)
        for (uint32_t s = 0; s < lay.m; s++)
            stored[r * lay.row_bytes() + lay.pos(s)] |= (uint8_t)(codes[r * lay.m + s] << lay.shift(s));
}

/// the product-quantised codes of the index, n x m in natural order
std::vector<uint8_t> host_pq_codes(const msvs_graph_index & ix, hipStream_t stream)
{
    const GraphPqLayout lay = ix.pq_layout();
    std::vector<uint8_t> stored(ix.n * lay.row_bytes()), out(ix.n * ix.pq_m);
    if (!stored.empty())
        MSVS_HIP(hipMemcpyAsync(stored.data(), ix.codes.p, stored.size(), hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    pq_unpack_rows(lay, stored.data(), ix.n, out.data());
    return out;
}

/// the file's rows: a code a byte at 8 bits; at 4 bits ceil(m / 2) bytes, the even s in the low nibble, the pad nibble 0
std::vector<uint8_t> pq_file_rows(const std::vector<uint8_t> & codes, size_t n, size_t m, uint32_t bits)
{
    if (bits == 8)
        return codes;
    const size_t rb = ceil_div(m, (size_t)2);
    std::vector<uint8_t> out(n * rb, 0);
    for (size_t r = 0; r < n; r++)
        for (size_t s = 0; s < m; s++)
            out[r * rb + s / 2] |= (uint8_t)(codes[r * m + s] << ((s & 1) * 4));
    return out;
}

/// what a caller's or a file's structure must satisfy -> nullptr, or what is wrong with it
const char * graph_structure_error(const float * centroids, size_t nlist, size_t dim, const int32_t * seeds, const uint32_t * nbr, size_t n, uint32_t R)
{
    for (size_t i = 0; i < nlist * dim; i++)
        if (!std::isfinite(centroids[i]))
            return "a centroid is not finite";
    for (size_t l = 0; l < nlist; l++)
        if (seeds[l] < -1 || (seeds[l] >= 0 && (size_t)seeds[l] >= n))
            return "a seed is outside [-1, n)";
    for (size_t e = 0; e < n * R; e++)
        if (nbr[e] != GRAPH_EMPTY && nbr[e] >= n)
            return "an edge is neither below n nor 0xFFFFFFFF";
    return nullptr;
}

std::vector<float> host_centroids(const msvs_graph_index & ix, hipStream_t stream)
{
    std::vector<float> c(ix.nlist * ix.dim);
    MSVS_HIP(hipMemcpy2DAsync(c.data(), ix.dim * 4, ix.centroids.p, (size_t)ix.ld * 4, ix.dim * 4, ix.nlist, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    return c;
}

struct GraphHeader // 64 bytes, little endian
{
    char magic[8]; // "MSVSGR01"
    uint32_t version; // 1: f32 rows of the store; 2: bit_size=8, the body continues with vmin, vmax and n x dim codes; 3: pq_m; 4: bit_size=16,
                      // the body continues with n x dim binary16 values
    int32_t metric;
    uint64_t dim, nlist, n, degree;
    uint64_t body; // FNV-1a of the centroids, the seeds and the edges (version 2: and vmin, vmax, the codes)
    uint64_t check; // FNV-1a of the bytes before it
};

uint64_t graph_body_check(const std::vector<float> & c, const std::vector<int32_t> & s, const std::vector<uint32_t> & e)
{
    const uint64_t h[3] = {fnv1a(c.data(), c.size() * 4), fnv1a(s.data(), s.size() * 4), fnv1a(e.data(), e.size() * 4)};
    return fnv1a(h, sizeof(h));
}

uint64_t graph_body_check2(const std::vector<float> & c, const std::vector<int32_t> & s, const std::vector<uint32_t> & e, const std::vector<float> & lo,
                           const std::vector<float> & hi, const std::vector<uint8_t> & codes)
{
    const uint64_t h[6] = {fnv1a(c.data(), c.size() * 4), fnv1a(s.data(), s.size() * 4), fnv1a(e.data(), e.size() * 4),
                           fnv1a(lo.data(), lo.size() * 4), fnv1a(hi.data(), hi.size() * 4), fnv1a(codes.data(), codes.size())};
    return fnv1a(h, sizeof(h));
}

/// version 3: the centroids, the seeds, the edges, (m, bits), the codebooks and the file's code rows
uint64_t graph_body_check3(const std::vector<float> & c, const std::vector<int32_t> & s, const std::vector<uint32_t> & e, const uint64_t (&geometry)[2],
                           const std::vector<float> & cb, const std::vector<uint8_t> & codes)
{
    const uint64_t h[6] = {fnv1a(c.data(), c.size() * 4), fnv1a(s.data(), s.size() * 4), fnv1a(e.data(), e.size() * 4),
                           fnv1a(geometry, sizeof(geometry)), fnv1a(cb.data(), cb.size() * 4), fnv1a(codes.data(), codes.size())};
    return fnv1a(h, sizeof(h));
}

/// version 4: the centroids, the seeds, the edges and the binary16 rows
uint64_t graph_body_check4(const std::vector<float> & c, const std::vector<int32_t> & s, const std::vector<uint32_t> & e, const std::vector<uint16_t> & rows)
{
    const uint64_t h[4] = {fnv1a(c.data(), c.size() * 4), fnv1a(s.data(), s.size() * 4), fnv1a(e.data(), e.size() * 4), fnv1a(rows.data(), rows.size() * 2)};
    return fnv1a(h, sizeof(h));
}
}

extern "C" int msvs_graph_index_create(int metric, const msvs_rows_t * rows, const char * params, msvs_graph_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        check_metric(metric, GRAPH);
        if (!rows)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null row store");
        const RowsView rv = rows_view(rows);
        if ((metric == MSVS_METRIC_COSINE) != (rv.normalize != 0))
            fail(MSVS_ERR_INVALID_ARGUMENT, "a cosine graph index needs a row store created with normalize=1, L2 and IP one with normalize=0");
        const auto p = parse_params(params);
        check_ncentroids(p);
        const long degree = param_int(p, "degree", 32);
        if (degree != 16 && degree != 32 && degree != 64)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index has degree 16, 32 or 64 (degree %ld)", degree);
        const long pq_m = param_int(p, "pq_m", 0);
        if (pq_m < 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "pq_m is 0 (off) or the number of sub-quantisers (pq_m %ld)", pq_m);
        const long bits = param_int(p, "bit_size", pq_m ? 8 : 32);
        if (!pq_m && bits != 32 && bits != 16 && bits != 8)
            fail(MSVS_ERR_INVALID_ARGUMENT,
                 "the graph index scores f32 rows (bit_size=32), binary16 rows (bit_size=16) or 8-bit codes (bit_size=8) (bit_size %ld)", bits);
        if (pq_m)
        {
            // (the smallest narrow search: ef = nprobe = width = max_iters = 1 reaches 1 + degree labels)
            const uint32_t tab = 2 * std::max<uint32_t>(1 + (uint32_t)degree, 32);
            if ((bits != 8 && bits != 4) || pq_m > 1024 / bits || rv.dim % (size_t)pq_m != 0
                || graph_pq_lds_bytes((uint32_t)pq_m, (uint32_t)bits, tab) > GRAPH_LDS_MAX)
                fail(MSVS_ERR_INVALID_ARGUMENT,
                     "a product-quantised graph index needs bit_size 8 or 4, 1 <= pq_m <= 128 (256 at bit_size=4) dividing dim, and tables "
                     "of pq_m KiB (pq_m / 16 KiB) + 7 KiB within 160 KiB (dim %zu, pq_m %ld, bit_size %ld)",
                     rv.dim, pq_m, bits);
        }
        const long join_iters = param_int(p, "join_iters", 0), build_nprobe = param_int(p, "build_nprobe", 8), join_sample = param_int(p, "join_sample", 8);
        if (join_iters < 0 || join_iters > 16)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the graph build runs 0 to 16 join iterations (join_iters %ld)", join_iters);
        if (join_iters && (build_nprobe < 1 || join_sample < 1 || join_sample > 32))
            fail(MSVS_ERR_INVALID_ARGUMENT, "the join needs build_nprobe >= 1 and 1 <= join_sample <= 32 (build_nprobe %ld, join_sample %ld)",
                 build_nprobe, join_sample);
        if (join_iters)
        {
            const uint32_t K0 = 2 * (uint32_t)degree, cap = K0 * ((uint32_t)join_sample + 1);
            const size_t lds = graph_join_lds_bytes(rv.ld / 4, K0, cap, graph_join_table(cap));
            if (lds > GRAPH_LDS_MAX)
                fail(MSVS_ERR_INVALID_ARGUMENT, "the graph join's LDS image (%zu bytes) exceeds %zu", lds, GRAPH_LDS_MAX);
        }
        std::unique_ptr<msvs_graph_index> ix(new msvs_graph_index);
        if (join_iters)
        {
            ix->join_iters = (size_t)join_iters;
            ix->build_nprobe = (size_t)build_nprobe;
            ix->join_sample = (uint32_t)join_sample;
        }
        ix->metric = metric;
        ix->dim = rv.dim;
        ix->ld = rv.ld;
        ix->bits = (uint32_t)bits;
        ix->pq_m = (size_t)pq_m;
        ix->ldc =(uint32_t)round_up(rv.dim, (size_t)16);
        ix->R = (uint32_t)degree;
        ix->rows = rows;
        ix->device = rv.device;
        ix->params = params ? params : "";
        *out = ix.release();
    });
}

extern "C" void msvs_graph_index_free(msvs_graph_index_t * ix) { delete ix; }
extern "C" int msvs_graph_index_ready(const msvs_graph_index_t * ix) { return ix && ix->ready ? 1 : 0; }
extern "C" size_t msvs_graph_index_num_data(const msvs_graph_index_t * ix) { return ix && ix->ready ? ix->n : 0; }
extern "C" size_t msvs_graph_index_num_lists(const msvs_graph_index_t * ix) { return ix ? ix->nlist : 0; }
extern "C" size_t msvs_graph_index_degree(const msvs_graph_index_t * ix) { return ix ? ix->R : 0; }
extern "C" size_t msvs_graph_index_bit_size(const msvs_graph_index_t * ix) { return ix ? ix->bits : 0; }
extern "C" size_t msvs_graph_index_memory_usage(const msvs_graph_index_t * ix)
{
    if (!ix)
        return 0;
    size_t coded = ix->sq() && ix->ready ? ix->n * ix->ldc + ix->d_vmin.bytes() + ix->d_step.bytes() : 0;
    if (ix->pq_m && ix->ready)
        coded = ix->n * ix->pq_layout().row_bytes() + ix->cbT.bytes();
    if (ix->h16() && ix->ready)
        coded = ix->n * ix->ldc * 2;
    return ix->nbr.bytes() + ix->centroids.bytes() + ix->seeds.bytes() + coded;
}
extern "C" size_t msvs_graph_index_pq_m(const msvs_graph_index_t * ix) { return ix ? ix->pq_m : 0; }

extern "C" int msvs_graph_index_set_pq_codebooks(msvs_graph_index_t * ix, const float * codebooks, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_graph_pq(*ix);
        if (!codebooks)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null codebooks");
        if (ix->ready)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index has its codes already: codebooks are handed in before build / set_graph");
        std::vector<float> cb(ix->ksub() * ix->dim);
        if (mem == MSVS_MEM_DEVICE)
            MSVS_HIP(hipMemcpy(cb.data(), codebooks, cb.size() * 4, hipMemcpyDeviceToHost));
        else
            memcpy(cb.data(), codebooks, cb.size() * 4);
        ix->cb_handed = false; // (a refused set leaves the index without codebooks)
        ix->h_cb.clear();
        ix->cbT.release();
        const size_t bad = first_non_finite(cb.data(), cb.size()), dsub = ix->dim / ix->pq_m;
        if (bad < cb.size())
            fail(MSVS_ERR_INVALID_ARGUMENT, "codebook entry %zu of sub-quantiser %zu is not finite", (bad / dsub) % ix->ksub(),
                 bad / (ix->ksub() * dsub));
        set_graph_codebooks(*ix, cb.data(), thread_stream());
        ix->cb_handed = true;
    });
}

extern "C" int msvs_graph_index_set_graph(msvs_graph_index_t * ix, const float * centroids, size_t nlist, const int32_t * seeds, const uint32_t * nbr,
                                          int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        if (!ix->rows)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index was loaded without a row store: nothing to make a graph over");
        const size_t n = msvs_rows_num(ix->rows);
        if (!centroids || !seeds || (n && !nbr) || nlist == 0 || nlist > 0x7fffffffull)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null graph / no centroids");
        std::vector<float> c(nlist * ix->dim);
        std::vector<int32_t> s(nlist);
        std::vector<uint32_t> e(n * ix->R);
        auto take = [&](void * dst, const void * src, size_t bytes) {
            if (mem == MSVS_MEM_DEVICE)
                MSVS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            else
                memcpy(dst, src, bytes);
        };
        take(c.data(), centroids, c.size() * 4);
        take(s.data(), seeds, s.size() * 4);
        if (!e.empty())
            take(e.data(), nbr, e.size() * 4);
        if (const char * bad = graph_structure_error(c.data(), nlist, ix->dim, s.data(), e.data(), n, ix->R))
            fail(MSVS_ERR_INVALID_ARGUMENT, "set_graph: %s", bad);
        ix->ready = false;
        ix->n = n;
        install_graph(*ix, c.data(), nlist, s.data(), e.data(), thread_stream());
        if (ix->pq_m)
            encode_pq_store(*ix, thread_stream());
        else if (ix->bits == 8)
            encode_store(*ix, thread_stream());
        else if (ix->bits == 16)
            encode_h16_store(*ix, thread_stream());
        ix->ready = true;
    });
}

/// Deterministic (include/msvs.h).  join_iters = 0: from exact lists, O(n^2) -- every row is searched over all rows.  join_iters >= 1:
/// from the lists of an IVFFLAT search of build_nprobe lists, repaired across partition borders by graph_join_kernel.
extern "C" int msvs_graph_index_build(msvs_graph_index_t * ix)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        if (!ix->rows)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the graph index was loaded without a row store: nothing to build a graph over");
        const RowsView rv = rows_view(ix->rows);
        const size_t n = rv.n, dim = ix->dim;
        const uint32_t R = ix->R, K0 = 2 * R;
        if (n == 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the row store is empty: nothing to build a graph over");
        hipStream_t stream = thread_stream();
        ix->ready = false;
        // the store's rows, dense, on the device: the trainer's and the FLAT index's feed, and the lists' queries
        DevBuf<float> dense(n * dim);
        MSVS_HIP(hipMemcpy2DAsync(dense.p, dim * 4, rv.host ? rv.host : rv.table, (size_t)rv.ld * 4, dim * 4, n, hipMemcpyDefault, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        // 1. centroids: the IVFFLAT trainer as it is
        {
            const TmpIndex tmp = kmeans(ix->metric, dim, ix->params, dense.p, n, MSVS_MEM_DEVICE);
            ix->nlist = tmp->nlist;
            ix->centroids.alloc(ix->nlist * ix->ld);
            MSVS_HIP(hipMemsetAsync(ix->centroids.p, 0, ix->nlist * ix->ld * 4, stream));
            MSVS_HIP(hipMemcpy2DAsync(ix->centroids.p, (size_t)ix->ld * 4, tmp->centroids.p, (size_t)tmp->ld * 4, dim * 4, ix->nlist,
                                      hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        const size_t nlist = ix->nlist, T = ix->join_iters;
        // the lists' search: a temporary index over the same rows (cosine: inner product over the stored unit rows, the queries
        // normalised here) -- FLAT, or with join_iters >= 1 IVFFLAT over the centroids of step 1, probing build_nprobe lists
        const int tmp_metric = ix->metric == MSVS_METRIC_L2 ? MSVS_METRIC_L2 : MSVS_METRIC_IP;
        msvs_index_t * raw = nullptr;
        int rc = msvs_index_create(T ? MSVS_INDEX_IVFFLAT : MSVS_INDEX_FLAT, tmp_metric, dim, "", &raw);
        TmpIndex lists_index(raw, msvs_index_free);
        if (rc == MSVS_OK && T)
        {
            DevBuf<float> cd(nlist * dim);
            MSVS_HIP(hipMemcpy2DAsync(cd.p, dim * 4, ix->centroids.p, (size_t)ix->ld * 4, dim * 4, nlist, hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
            rc = msvs_index_set_centroids(raw, cd.p, nlist, MSVS_MEM_DEVICE);
        }
        if (rc == MSVS_OK)
            rc = msvs_index_add(raw, dense.p, nullptr, n, MSVS_MEM_DEVICE);
        if (rc == MSVS_OK)
            rc = msvs_index_build(raw);
        if (rc != MSVS_OK)
            fail(rc, "%s", std::string(msvs_last_error()).c_str());
        const size_t chunk = std::max(GRAPH_LIST_CHUNK, nlist), lists_nprobe = T ? std::min(ix->build_nprobe, nlist) : 1;
        DevBuf<float> dq(chunk * dim), ddis(chunk * (K0 + 1));
        DevBuf<int64_t> dids(chunk * (K0 + 1));
        auto as_queries = [&](const float * src, size_t src_ld, size_t cnt, float * dst, size_t dst_ld) {
            if (dst_ld != dim)
                MSVS_HIP(hipMemsetAsync(dst, 0, cnt * dst_ld * 4, stream));
            MSVS_HIP(hipMemcpy2DAsync(dst, dst_ld * 4, src, src_ld * 4, dim * 4, cnt, hipMemcpyDeviceToDevice, stream));
            if (ix->metric == MSVS_METRIC_COSINE)
                normalize_device_rows(dst, cnt, (uint32_t)dim, (uint32_t)dst_ld, stream);
        };
        auto exact = [&](const float * src, size_t src_ld, size_t cnt, uint32_t k) {
            as_queries(src, src_ld, cnt, dq.p, dim);
            rc = msvs_index_search_device(raw, dq.p, cnt, (int)k, (int)lists_nprobe, nullptr, 0, dids.p, ddis.p, stream);
            if (rc != MSVS_OK)
                fail(rc, "%s", std::string(msvs_last_error()).c_str());
        };
        // the join's rows: a device table with the store's leading dimension -- the store's own when it is in HBM, else a padded copy
        DevBuf<float> padded;
        const float * table = rv.table;
        if (T && rv.host)
        {
            table = dense.p;
            if (ix->ld != dim)
            {
                padded.alloc(n * ix->ld);
                upload_rows(padded.p, dense.p, n, (uint32_t)dim, ix->ld, MSVS_MEM_DEVICE, stream);
                table = padded.p;
            }
        }
        // 2. seeds: the exact top-1 of every centroid (join_iters >= 1: the canonical scan over the join's table, as the coarse step)
        if (T)
        {
            DevBuf<float> cq(nlist * ix->ld);
            as_queries(ix->centroids.p, ix->ld, nlist, cq.p, ix->ld);
            Scratch & scr = scratch_for(stream);
            scr.reserve(flat_scratch_bytes(n, nlist, 1, ix->ld) + 1024, stream);
            MergeParams out{};
            out.out_ids = dids.p;
            out.out_dis = ddis.p;
            flat_search_device(scr, scan_metric(ix->metric), table, nullptr, n, ix->ld, cq.p, nlist, 1, nullptr, 0, out, stream);
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        else
            exact(ix->centroids.p, ix->ld, nlist, 1);
        std::vector<int64_t> top(nlist);
        MSVS_HIP(hipMemcpyAsync(top.data(), dids.p, nlist * 8, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        std::vector<int32_t> seeds(nlist);
        for (size_t l = 0; l < nlist; l++)
            seeds[l] = top[l] >= 0 && (size_t)top[l] < n ? (int32_t)top[l] : -1;
        // 3. lists: the exact top-(K0 + 1) of every row, the row itself taken out
        DevBuf<int32_t> lists(n * K0);
        for (size_t i0 = 0; i0 < n; i0 += chunk)
        {
            const size_t cnt = std::min(chunk, n - i0);
            exact(dense.p + i0 * dim, dim, cnt, K0 + 1);
            hipLaunchKernelGGL(graph_lists_kernel, dim3((unsigned)ceil_div(cnt, (size_t)256)), dim3(256), 0, stream, dids.p, (uint32_t)cnt, (uint32_t)i0,
                               K0, lists.p);
            MSVS_HIP(hipGetLastError());
        }
        // 3b, 3c. the join: T iterations at most, old lists in, new lists out, until no list changes
        const int32_t * final_lists = lists.p;
        DevBuf<int32_t> other;
        if (T)
        {
            other.alloc(n * K0);
            DevBuf<uint32_t> changed(1);
            DevBuf<float> jq(ix->metric == MSVS_METRIC_COSINE ? std::min(n, GRAPH_QUERY_CHUNK) * ix->ld : 0);
            GraphJoinParams a{};
            a.rows = reinterpret_cast<const float4 *>(table);
            a.changed = changed.p;
            a.n = (uint32_t)n;
            a.ld4 = ix->ld / 4;
            a.K0 = K0;
            a.S = ix->join_sample;
            a.cap = K0 * (ix->join_sample + 1);
            a.tab = graph_join_table(a.cap);
            const size_t lds = graph_join_lds_bytes(a.ld4, K0, a.cap, a.tab), step = jq.n ? GRAPH_QUERY_CHUNK : n;
            int32_t * bufs[2] = {lists.p, other.p};
            for (size_t t = 0; t < T; t++)
            {
                a.lists = bufs[t & 1];
                a.next = bufs[(t + 1) & 1];
                MSVS_HIP(hipMemsetAsync(changed.p, 0, 4, stream));
                for (size_t i0 = 0; i0 < n; i0 += step) // (cosine: the nodes' rows normalised again, a chunk at a time)
                {
                    const size_t cnt = std::min(step, n - i0);
                    if (jq.n)
                        as_queries(table + i0 * ix->ld, ix->ld, cnt, jq.p, ix->ld);
                    a.Q = reinterpret_cast<const float4 *>(jq.n ? jq.p : table + i0 * ix->ld);
                    a.i0 = (uint32_t)i0;
                    ProfileScope prof("graph_join", stream);
                    with_int<M_IP, M_L2>(scan_metric(ix->metric), [&](auto mm) { launch_graph_join<decltype(mm)::value>(a, cnt, lds, stream); });
                    MSVS_HIP(hipGetLastError());
                }
                uint32_t moved = 0;
                MSVS_HIP(hipMemcpyAsync(&moved, changed.p, 4, hipMemcpyDeviceToHost, stream));
                MSVS_HIP(hipStreamSynchronize(stream));
                final_lists = a.next;
                if (moved == 0)
                    break;
            }
            lists_index.reset(); // (the stream is idle)
        }
        // 4. prune by detours; 5. reverse edges: count, prefix sum, scatter, per-node selection and merge
        const size_t words = n * R;
        DevBuf<uint32_t> F(words), cnt(n);
        DevBuf<uint64_t> off(n + 1), seg(words);
        ix->nbr.alloc(words);
        static std::once_flag once;
        std::call_once(once, [] {
            MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&graph_prune_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)graph_prune_lds_bytes(128)));
        });
        hipLaunchKernelGGL(graph_prune_kernel, dim3((unsigned)n), dim3(BLOCK), graph_prune_lds_bytes(K0), stream, final_lists, (uint32_t)n, K0, R, F.p);
        MSVS_HIP(hipMemsetAsync(cnt.p, 0, n * 4, stream));
        const unsigned egrid = (unsigned)ceil_div(words, (size_t)256);
        hipLaunchKernelGGL(graph_count_kernel, dim3(egrid), dim3(256), 0, stream, F.p, words, cnt.p);
        hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, cnt.p, (uint32_t)n, off.p);
        hipLaunchKernelGGL(graph_scatter_kernel, dim3(egrid), dim3(256), 0, stream, F.p, words, log2_of(R), off.p, cnt.p, seg.p);
        hipLaunchKernelGGL(graph_reverse_kernel, dim3((unsigned)ceil_div(n, (size_t)4)), dim3(BLOCK), 0, stream, F.p, off.p, seg.p, (uint32_t)n, R,
                           ix->nbr.p);
        MSVS_HIP(hipGetLastError());
        ix->seeds.alloc(nlist);
        MSVS_HIP(hipMemcpyAsync(ix->seeds.p, seeds.data(), nlist * 4, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
        ix->n = n;
        if (ix->pq_m)
            encode_pq_store(*ix, stream);
        else if (ix->bits == 8)
            encode_store(*ix, stream);
        else if (ix->bits == 16)
            encode_h16_store(*ix, stream);
        ix->ready = true;
    });
}

/// search_device / search_wide_device
int graph_search_device_entry(const msvs_graph_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t ef, size_t nprobe, size_t width,
                              size_t max_iters, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream, bool wide)
{
    return guarded([&] {
        const size_t limit = wide ? MSVS_MAX_K_ROUNDS : MSVS_MAX_K;
        check_graph(ix);
        check_k(k, limit);
        (wide ? graph_wide_search_device : graph_search_device)(*ix, d_queries, nq, k, graph_defaults(k, ef, nprobe, width, max_iters, limit),
                                                                 d_alive_bits, nbits, d_ids, d_dis, as_stream(hip_stream));
    });
}

/// search / search_wide: the queries and the filter staged in, the results staged out
int graph_search_entry(const msvs_graph_index_t * ix, const float * queries, size_t nq, size_t k, const char * params, const uint64_t * alive_bits,
                       size_t nbits, int64_t * ids, float * dis, bool wide)
{
    return guarded([&] {
        const size_t limit = wide ? MSVS_MAX_K_ROUNDS : MSVS_MAX_K;
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_k(k, limit);
        const GraphSearch s = parse_graph_search(params, k, limit);
        check_graph_ready(*ix);
        if (k > s.ef)
            fail(MSVS_ERR_UNSUPPORTED_K, "k = %zu exceeds ef = %zu, the beam of the graph search", k, s.ef);
        if (nq == 0 || k == 0)
            return;
        if (!queries || !ids || !dis)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
        hipStream_t stream = thread_stream();
        const size_t words = alive_bits ? std::max<size_t>(1, ceil_div(nbits, (size_t)64)) : 0;
        Scratch & stg = staging_for(stream);
        stg.reserve(nq * ix->dim * 4 + nq * k * 12 + words * 8 + 4 * 256, stream);
        float * dq = stg.take<float>(nq * ix->dim);
        int64_t * d_ids = stg.take<int64_t>(nq * k);
        float * d_dis = stg.take<float>(nq * k);
        uint64_t * d_alive = words ? stg.take<uint64_t>(words) : nullptr;
        MSVS_HIP(hipMemcpyAsync(dq, queries, nq * ix->dim * 4, hipMemcpyHostToDevice, stream));
        if (words)
            MSVS_HIP(hipMemcpyAsync(d_alive, alive_bits, words * 8, hipMemcpyHostToDevice, stream));
        (wide ? graph_wide_search_device : graph_search_device)(*ix, dq, nq, k, s, d_alive, nbits, d_ids, d_dis, stream);
        MSVS_HIP(hipMemcpyAsync(ids, d_ids, nq * k * 8, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipMemcpyAsync(dis, d_dis, nq * k * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
    });
}

extern "C" int msvs_graph_index_search_device(const msvs_graph_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t ef, size_t nprobe,
                                              size_t width, size_t max_iters, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                              float * d_dis, void * hip_stream)
{
    return graph_search_device_entry(ix, d_queries, nq, k, ef, nprobe, width, max_iters, d_alive_bits, nbits, d_ids, d_dis, hip_stream, false);
}

extern "C" int msvs_graph_index_search(const msvs_graph_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                       const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return graph_search_entry(ix, queries, nq, k, params, alive_bits, nbits, ids, dis, false);
}

extern "C" int msvs_graph_index_search_wide_device(const msvs_graph_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t ef,
                                                   size_t nprobe, size_t width, size_t max_iters, const uint64_t * d_alive_bits, size_t nbits,
                                                   int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return graph_search_device_entry(ix, d_queries, nq, k, ef, nprobe, width, max_iters, d_alive_bits, nbits, d_ids, d_dis, hip_stream, true);
}

extern "C" int msvs_graph_index_search_wide(const msvs_graph_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                            const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return graph_search_entry(ix, queries, nq, k, params, alive_bits, nbits, ids, dis, true);
}

// ------------------------------------------------------------------------------------------- export and files

extern "C" int msvs_graph_index_export(const msvs_graph_index_t * ix, float * centroids, int32_t * seeds, uint32_t * nbr)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_graph_ready(*ix);
        hipStream_t stream = thread_stream();
        if (centroids)
        {
            const std::vector<float> c = host_centroids(*ix, stream);
            memcpy(centroids, c.data(), c.size() * 4);
        }
        if (seeds)
            MSVS_HIP(hipMemcpyAsync(seeds, ix->seeds.p, ix->nlist * 4, hipMemcpyDeviceToHost, stream));
        if (nbr && ix->n)
            MSVS_HIP(hipMemcpyAsync(nbr, ix->nbr.p, ix->n * ix->R * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
    });
}

extern "C" int msvs_graph_index_export_codes(const msvs_graph_index_t * ix, float * vmin, float * vmax, uint8_t * codes)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_graph_coded(*ix);
        check_graph_ready(*ix);
        if (vmin)
            memcpy(vmin, ix->h_vmin.data(), ix->dim * 4);
        if (vmax)
            memcpy(vmax, ix->h_vmax.data(), ix->dim * 4);
        if (codes)
        {
            const std::vector<uint8_t> c = host_codes(*ix, thread_stream());
            memcpy(codes, c.data(), c.size());
        }
    });
}

extern "C" int msvs_graph_index_export_pq(const msvs_graph_index_t * ix, float * codebooks, uint8_t * codes)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_graph_pq(*ix);
        check_graph_ready(*ix);
        if (codebooks)
            memcpy(codebooks, ix->h_cb.data(), ix->h_cb.size() * 4);
        if (codes)
        {
            const std::vector<uint8_t> c = host_pq_codes(*ix, thread_stream());
            memcpy(codes, c.data(), c.size());
        }
    });
}

extern "C" int msvs_graph_index_serialize_io(const msvs_graph_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_graph(ix);
        check_graph_ready(*ix);
        hipStream_t stream = thread_stream();
        const std::vector<float> c = host_centroids(*ix, stream);
        std::vector<int32_t> s(ix->nlist);
        std::vector<uint32_t> e(ix->n * ix->R);
        MSVS_HIP(hipMemcpy(s.data(), ix->seeds.p, s.size() * 4, hipMemcpyDeviceToHost));
        if (!e.empty())
            MSVS_HIP(hipMemcpy(e.data(), ix->nbr.p, e.size() * 4, hipMemcpyDeviceToHost));
        const bool coded = ix->sq(), pq = ix->pq_m != 0;
        const std::vector<uint8_t> codes = coded ? host_codes(*ix, stream)
                                           : pq  ? pq_file_rows(host_pq_codes(*ix, stream), ix->n, ix->pq_m, ix->bits)
                                                 : std::vector<uint8_t>();
        const bool h16 = ix->h16();
        const std::vector<uint16_t> halves = h16 ? host_h16_rows(*ix, stream) : std::vector<uint16_t>();
        const uint64_t geometry[2] = {ix->pq_m, ix->bits};
        IoStream f(io, "graph_data", 1);
        GraphHeader h{};
        memcpy(h.magic, "MSVSGR01", 8);
        h.version = h16 ? 4 : pq ? 3 : coded ? 2 : 1;
        h.metric = ix->metric;
        h.dim = ix->dim;
        h.nlist = ix->nlist;
        h.n = ix->n;
        h.degree = ix->R;
        h.body = h16     ? graph_body_check4(c, s, e, halves)
                 : pq    ? graph_body_check3(c, s, e, geometry, ix->h_cb, codes)
                 : coded ? graph_body_check2(c, s, e, ix->h_vmin, ix->h_vmax, codes)
                         : graph_body_check(c, s, e);
        h.check = fnv1a(&h, offsetof(GraphHeader, check));
        f.write(&h, sizeof(h));
        f.write(c.data(), c.size() * 4);
        f.write(s.data(), s.size() * 4);
        if (!e.empty())
            f.write(e.data(), e.size() * 4);
        if (h16 && !halves.empty())
            f.write(halves.data(), halves.size() * 2);
        if (pq)
        {
            f.write(geometry, sizeof(geometry));
            f.write(ix->h_cb.data(), ix->h_cb.size() * 4);
            if (!codes.empty())
                f.write(codes.data(), codes.size());
        }
        if (coded)
        {
            f.write(ix->h_vmin.data(), ix->dim * 4);
            f.write(ix->h_vmax.data(), ix->dim * 4);
            if (!codes.empty())
                f.write(codes.data(), codes.size());
        }
        f.finish();
    });
}

extern "C" int msvs_graph_index_load_io(const msvs_io_t * io, const msvs_rows_t * rows, msvs_graph_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        int device = 0;
        MSVS_HIP(hipGetDevice(&device));
        RowsView rv{};
        if (rows)
            rv = rows_view(rows);
        DeviceGuard on_device(rows ? rv.device : device);
        std::unique_ptr<msvs_graph_index> ix(new msvs_graph_index);
        std::vector<float> c, lo, hi;
        std::vector<int32_t> s;
        std::vector<uint32_t> e;
        std::vector<uint8_t> codes;
        IoStream f(io, "graph_data", 0);
        GraphHeader h{};
        f.read(&h, sizeof(h));
        if (memcmp(h.magic, "MSVSGR01", 8) != 0 || h.version < 1 || h.version > 4 || h.check != fnv1a(&h, offsetof(GraphHeader, check))
            || !header_ranges_ok(h.metric, h.dim, h.nlist, h.n) || (h.degree != 16 && h.degree != 32 && h.degree != 64))
            fail(MSVS_ERR_IO, "corrupt msvs graph index header");
        const bool pq = h.version == 3, h16 = h.version == 4, coded = h.version >= 2; // (coded: the file carries what the search reads)
        if (!coded && !rows)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null row store: only a file of a bit_size=8, bit_size=16 or pq_m index carries what its search reads");
        if (coded && h.dim == 0)
            fail(MSVS_ERR_IO, "corrupt msvs graph index header");
        if (coded ? (rows && h.n != rv.n) : (h.n != rv.n || h.dim != rv.dim || (h.metric == MSVS_METRIC_COSINE) != (rv.normalize != 0)))
            fail(MSVS_ERR_IO, "the msvs graph index file (n %llu, dim %llu) does not belong to this row store (n %zu, dim %zu)",
                 (unsigned long long)h.n, (unsigned long long)h.dim, rv.n, rv.dim);
        read_grow(f, c, (size_t)(h.nlist * h.dim));
        read_grow(f, s, (size_t)h.nlist);
        read_grow(f, e, (size_t)(h.n * h.degree));
        uint64_t geometry[2] = {0, 0}; // version 3: m, bits
        std::vector<float> cb;
        std::vector<uint16_t> halves; // version 4
        if (h16)
            read_grow(f, halves, (size_t)(h.n * h.dim));
        else if (pq)
        {
            f.read(geometry, sizeof(geometry));
            const uint64_t m = geometry[0], bits = geometry[1];
            if ((bits != 8 && bits != 4) || m < 1 || m > 1024 / bits || h.dim % m != 0)
                fail(MSVS_ERR_IO, "corrupt msvs graph index: %llu sub-quantisers of %llu bits over dim %llu", (unsigned long long)m,
                     (unsigned long long)bits, (unsigned long long)h.dim);
            read_grow(f, cb, (size_t)(h.dim << bits));
            read_grow(f, codes, (size_t)(h.n * ceil_div(m * bits, (uint64_t)8)));
        }
        else if (coded)
        {
            read_grow(f, lo, (size_t)h.dim);
            read_grow(f, hi, (size_t)h.dim);
            read_grow(f, codes, (size_t)(h.n * h.dim));
        }
        expect_end(f);
        if (h.body != (h16 ? graph_body_check4(c, s, e, halves) : pq ? graph_body_check3(c, s, e, geometry, cb, codes) : coded ? graph_body_check2(c, s, e, lo, hi, codes) : graph_body_check(c, s, e)))
            fail(MSVS_ERR_IO, "corrupt msvs graph index: the body's checksum does not match");
        if (pq && first_non_finite(cb.data(), cb.size()) < cb.size())
            fail(MSVS_ERR_IO, "corrupt msvs graph index: a codebook entry is not finite");
        if (pq && geometry[1] == 4 && (geometry[0] & 1)) // (a code is a nibble or a byte: none can reach ksub; the pad nibble can be set)
            for (size_t r = 0, rb = (size_t)(geometry[0] + 1) / 2; r < h.n; r++)
                if (codes[r * rb + rb - 1] >> 4)
                    fail(MSVS_ERR_IO, "corrupt msvs graph index: the pad nibble of row %zu is not 0", r);
        if (const char * bad = graph_structure_error(c.data(), (size_t)h.nlist, (size_t)h.dim, s.data(), e.data(), (size_t)h.n, (uint32_t)h.degree))
            fail(MSVS_ERR_IO, "corrupt msvs graph index: %s", bad);
        if (coded && !pq && !h16)
            for (size_t j = 0; j < h.dim; j++)
                if (graph_unusable_dimension(&lo[j], &hi[j], 1) == 0 || hi[j] < lo[j])
                    fail(MSVS_ERR_IO, "corrupt msvs graph index: the quantiser bounds of dimension %zu are not finite, vmax < vmin or their span is infinite", j);
        ix->metric = h.metric;
        ix->dim = (size_t)h.dim;
        ix->ld = padded_dim((size_t)h.dim);
        ix->bits = pq ? (uint32_t)geometry[1] : h16 ? 16 : coded ? 8 : 32;
        ix->pq_m = (size_t)geometry[0];
        ix->ldc = (uint32_t)round_up((size_t)h.dim, (size_t)16);
        ix->R = (uint32_t)h.degree;
        // (a version-2 file is checked against a store for n alone; build / set_graph need one of the index's own shape)
        ix->rows = rows && rv.dim == h.dim && (h.metric == MSVS_METRIC_COSINE) == (rv.normalize != 0) ? rows : nullptr;
        ix->device = rows ? rv.device : device;
        ix->n = (size_t)h.n;
        hipStream_t stream = thread_stream();
        install_graph(*ix, c.data(), (size_t)h.nlist, s.data(), e.data(), stream);
        if (pq)
        {
            set_graph_codebooks(*ix, cb.data(), stream);
            ix->cb_handed = true; // (a later set_graph over a store encodes with the file's codebooks)
            const GraphPqLayout lay = ix->pq_layout();
            std::vector<uint8_t> natural(ix->n * ix->pq_m), stored(std::max<size_t>(ix->n * lay.row_bytes(), 1), 0);
            const size_t rb = codes.size() / std::max<size_t>(ix->n, 1);
            for (size_t r = 0; r < ix->n; r++)
                for (size_t s = 0; s < ix->pq_m; s++)
                    natural[r * ix->pq_m + s] = ix->bits == 8 ? codes[r * rb + s] : (codes[r * rb + s / 2] >> ((s & 1) * 4)) & 15;
            pq_pack_rows(lay, natural.data(), ix->n, stored.data());
            ix->codes.alloc(stored.size());
            MSVS_HIP(hipMemcpy(ix->codes.p, stored.data(), stored.size(), hipMemcpyHostToDevice));
        }
        else if (h16)
        {
            std::vector<uint16_t> stored(std::max<size_t>(ix->n * ix->ldc, 1), 0); // natural order -> the stored order, pad halves 0
            for (size_t r = 0; r < ix->n; r++)
                for (size_t j = 0; j < ix->dim; j++)
                    stored[r * ix->ldc + h16_stored_pos(j, ix->ldc)] = halves[r * ix->dim + j];
            ix->codes.alloc(stored.size() * 2);
            MSVS_HIP(hipMemcpy(ix->codes.p, stored.data(), stored.size() * 2, hipMemcpyHostToDevice));
        }
        else if (coded)
        {
            set_graph_quantiser(*ix, lo.data(), hi.data(), stream);
            std::vector<uint8_t> stored(std::max<size_t>(ix->n * ix->ldc, 1), 0); // natural order -> the stored order, pad bytes 0
            for (size_t r = 0; r < ix->n; r++)
                for (size_t j = 0; j < ix->dim; j++)
                    stored[r * ix->ldc + sq_stored_pos((uint32_t)j, ix->ldc)] = codes[r * ix->dim + j];
            ix->codes.alloc(stored.size());
            MSVS_HIP(hipMemcpy(ix->codes.p, stored.data(), stored.size(), hipMemcpyHostToDevice));
        }
        ix->ready = true;
        *out = ix.release();
    });
}
