// coded_ivf.hpp -- the host code the IVFSQ and IVFPQ indexes share (sq_index.hip, pq_index.hip): both are coarse centroids, staged
// chunks of (codes, list, label), a list-major build, u32 labels, the grouped list scan (coarse top-P, GroupedPlan, a scan kernel,
// launch_ivf_merge) and a two-file format with FNV-1a header checks; they differ in the code word.  What differs comes in as a
// callable (a lambda at the call site) or a plain argument; `name` is "IVFSQ" / "IVFPQ" for the messages.
// Reused as they are: the k-means trainer (temporary IVFFLAT indexes), the assignment kernel, flat_search_device for the coarse
// step, GroupedPlan, plan_segments, launch_ivf_merge, launch_round_scatter, Scratch, normalize_device_rows, upload_rows, list_major_layout.
// Also here: the two-stage search both indexes offer (search_refine_device: their own search, then refine.hip's exact re-rank).
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "index_internal.hpp"
#include "io_stream.hpp"
#include "ivf_build_kernels.hpp"
#include "list_layout.hpp"

namespace msvs
{
constexpr size_t CODED_ADD_ROWS = 65536;          // rows of a chunk on the device as f32 at a time (encode, range, residuals)
constexpr uint32_t CODED_LABEL_END = 0xffffffffu; // labels are < this

struct CodedIvf
{
    int metric = MSVS_METRIC_L2;
    size_t dim = 0;
    uint32_t ld = 0;        // floats per centroid / query row
    uint32_t row_bytes = 0; // bytes of a stored row
    int device = 0;
    std::string params; // create's, handed to the temporary IVFFLAT indexes that run the k-means
    // codebook (the coarse part)
    size_t nlist = 0;
    DevBuf<float> centroids;   // nlist x ld
    std::vector<float> h_cent; // nlist x dim
    bool trained = false;
    // staging (between add and build): codes, list and label only
    struct Chunk
    {
        DevBuf<uint8_t> codes; // n x row_bytes, stored order
        std::vector<int32_t> list;
        std::vector<int64_t> ids;
        size_t n = 0;
    };
    std::vector<Chunk> chunks;
    size_t staged = 0;
    // final storage
    DevBuf<uint8_t> codes;    // list-major rows of row_bytes (the index's own layout within)
    DevBuf<uint32_t> labels;  // n
    DevBuf<int64_t> list_off; // nlist + 1
    std::vector<int64_t> h_list_off;
    size_t n = 0, max_list_len = 0;
    bool ready = false;
};

// ------------------------------------------------------------------------------------------- checks

/// the out argument of create and load: must be there, and is null until the call has succeeded
template <class Index>
inline void clear_out(Index ** out)
{
    if (!out)
        fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
}

inline void check_index(const CodedIvf * ix)
{
    if (!ix)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
}

inline void check_rows(const CodedIvf * ix, const float * x, size_t n)
{
    if (!ix || (n && !x))
        fail(MSVS_ERR_INVALID_ARGUMENT, "null index / data");
}

inline void check_trained(const CodedIvf & ix, const char * name)
{
    if (!ix.trained)
        fail(MSVS_ERR_NOT_READY, "the %s index has no codebook yet (train / set_codebook)", name);
}

inline void check_built(const CodedIvf & ix, const char * name)
{
    if (!ix.ready)
        fail(MSVS_ERR_NOT_READY, "the %s index is not built", name);
}

inline void check_codebook_time(const CodedIvf & ix)
{
    if (ix.staged || ix.ready)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the codebook must be set before data is added");
}

inline bool metric_ok(int metric) { return metric == MSVS_METRIC_L2 || metric == MSVS_METRIC_IP || metric == MSVS_METRIC_COSINE; }

inline void check_metric(int metric, const char * name)
{
    if (!metric_ok(metric))
        fail(MSVS_ERR_NOT_IMPLEMENTED, "metric %d is not implemented for the %s index", metric, name);
}

inline void check_ncentroids(const std::map<std::string, std::string> & p)
{
    if (param_int(p, "ncentroids", 1024) < 1)
        fail(MSVS_ERR_INVALID_ARGUMENT, "bad ncentroids");
}

/// the ranges of a data-file header that do not depend on the code word
inline bool header_ranges_ok(int32_t metric, uint64_t dim, uint64_t nlist, uint64_t n)
{
    return metric_ok(metric) && dim <= 8192 && nlist != 0 && nlist <= 0x7fffffffull && n <= 0xfffffff0ull;
}

// ------------------------------------------------------------------------------------------- codebook

/// nearest centroid of n device rows (stride ld): by L2 for L2 indexes, by inner product for IP and cosine (as msvs_index_add)
inline void assign(const CodedIvf & ix, const float * d_x, size_t n, int32_t * d_assign, float * d_cnorm, hipStream_t stream)
{
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((unsigned)ceil_div(ix.nlist, (size_t)256)), dim3(256), 0, stream, ix.centroids.p, d_cnorm,
                       (uint32_t)ix.nlist, (uint32_t)ix.dim, ix.ld);
    const unsigned grid = (unsigned)ceil_div(n, (size_t)AS_TN);
    if (ix.metric == MSVS_METRIC_L2)
        hipLaunchKernelGGL((assign_kernel<false>), dim3(grid), dim3(256), 0, stream, d_x, n, ix.centroids.p, d_cnorm, (uint32_t)ix.nlist,
                           (uint32_t)ix.dim, ix.ld, d_assign, (float *)nullptr);
    else
        hipLaunchKernelGGL((assign_kernel<true>), dim3(grid), dim3(256), 0, stream, d_x, n, ix.centroids.p, d_cnorm, (uint32_t)ix.nlist,
                           (uint32_t)ix.dim, ix.ld, d_assign, (float *)nullptr);
    MSVS_HIP(hipGetLastError());
}

/// m rows of the caller's chunk (host or device, dense) -> stored rows on the device (padded, normalised for cosine) and their lists
inline void stage_rows(const CodedIvf & ix, const float * x, size_t m, int mem, float * d_x, int32_t * d_assign, float * d_cnorm,
                       hipStream_t stream)
{
    upload_rows(d_x, x, m, (uint32_t)ix.dim, ix.ld, mem, stream);
    if (ix.metric == MSVS_METRIC_COSINE)
        normalize_device_rows(d_x, m, (uint32_t)ix.dim, ix.ld, stream);
    assign(ix, d_x, m, d_assign, d_cnorm, stream);
}

using TmpIndex = std::unique_ptr<msvs_index_t, void (*)(msvs_index_t *)>;

/// a temporary IVFFLAT index trained on (x, n): the k-means as it is
inline TmpIndex kmeans(int metric, size_t dim, const std::string & params, const float * x, size_t n, int mem)
{
    msvs_index_t * tmp = nullptr;
    int rc = msvs_index_create(MSVS_INDEX_IVFFLAT, metric, dim, params.c_str(), &tmp);
    if (rc == MSVS_OK)
        rc = msvs_index_train(tmp, x, n, mem);
    if (rc != MSVS_OK)
    {
        const std::string why = msvs_last_error();
        msvs_index_free(tmp);
        fail(rc, "%s", why.c_str());
    }
    return TmpIndex(tmp, msvs_index_free);
}

/// the coarse centroids: the IVFFLAT trainer as it is, through a temporary index of the same metric and parameters, copied padded
inline void train_centroids(CodedIvf & ix, const float * x, size_t n, int mem, hipStream_t stream)
{
    const TmpIndex tmp = kmeans(ix.metric, ix.dim, ix.params, x, n, mem);
    ix.nlist = tmp->nlist;
    ix.centroids.alloc(ix.nlist * ix.ld);
    MSVS_HIP(hipMemsetAsync(ix.centroids.p, 0, ix.nlist * ix.ld * 4, stream));
    MSVS_HIP(hipMemcpy2DAsync(ix.centroids.p, (size_t)ix.ld * 4, tmp->centroids.p, (size_t)tmp->ld * 4, ix.dim * 4, ix.nlist,
                              hipMemcpyDeviceToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
}

/// nlist dense centroid rows (host or device) -> the padded device rows; ix.nlist is the caller's to set
inline void upload_centroids(CodedIvf & ix, const float * centroids, size_t nlist, int mem, hipStream_t stream)
{
    ix.centroids.alloc(nlist * ix.ld);
    upload_rows(ix.centroids.p, centroids, nlist, (uint32_t)ix.dim, ix.ld, mem, stream);
    MSVS_HIP(hipStreamSynchronize(stream));
}

/// the last step of setting a codebook: the centroids' host copy; synchronises, so the caller's upload buffers may go
inline void finish_codebook(CodedIvf & ix, hipStream_t stream)
{
    const size_t d = ix.dim;
    ix.h_cent.resize(ix.nlist * d);
    MSVS_HIP(hipMemcpy2DAsync(ix.h_cent.data(), d * 4, ix.centroids.p, (size_t)ix.ld * 4, d * 4, ix.nlist, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    ix.trained = true;
}

// ------------------------------------------------------------------------------------------- add and build

/// the labels of n added rows: the caller's (host or device) or the staged positions; all within the label range
inline std::vector<int64_t> take_ids(const CodedIvf & ix, const int64_t * ids, size_t n, int mem)
{
    std::vector<int64_t> out(n);
    if (ids)
    {
        if (mem == MSVS_MEM_DEVICE)
            MSVS_HIP(hipMemcpy(out.data(), ids, n * 8, hipMemcpyDeviceToHost));
        else
            memcpy(out.data(), ids, n * 8);
    }
    else
        for (size_t i = 0; i < n; i++)
            out[i] = (int64_t)(ix.staged + i);
    for (size_t i = 0; i < n; i++)
        if (out[i] < 0 || out[i] >= (int64_t)CODED_LABEL_END)
            fail(MSVS_ERR_ID_RANGE, "id %lld is outside the label range [0, 2^32 - 1)", (long long)out[i]);
    return out;
}

/// msvs_*_index_add but for the encode launch: encode(d_x, d_assign, cnt, dst, stream) enqueues it for cnt staged rows, dst
/// their stored rows
template <class Encode>
inline void add_rows(CodedIvf * ix, const float * x, const int64_t * ids, size_t n, int mem, const char * name, bool zero_chunk, Encode encode)
{
    DeviceGuard on_device(ix ? ix->device : -1);
    check_rows(ix, x, n);
    if (ix->ready)
        fail(MSVS_ERR_INVALID_ARGUMENT, "index already built");
    check_trained(*ix, name);
    if (n == 0)
        return;
    if (ix->staged + n > 0xfffffff0ull)
        fail(MSVS_ERR_ID_RANGE, "more rows than the u32 row range");
    hipStream_t stream = thread_stream();
    CodedIvf::Chunk ch;
    ch.n = n;
    ch.ids = take_ids(*ix, ids, n, mem);
    ch.codes.alloc(n * ix->row_bytes);
    if (zero_chunk)
        MSVS_HIP(hipMemsetAsync(ch.codes.p, 0, n * ix->row_bytes, stream)); // the padding bytes of a row are 0
    ch.list.resize(n);
    const size_t step_rows = std::min(n, CODED_ADD_ROWS);
    DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist);
    DevBuf<int32_t> d_assign(step_rows);
    for (size_t r0 = 0; r0 < n; r0 += step_rows)
    {
        const size_t cnt = std::min(step_rows, n - r0);
        stage_rows(*ix, x + r0 * ix->dim, cnt, mem, d_x.p, d_assign.p, d_cnorm.p, stream);
        encode(d_x.p, d_assign.p, cnt, ch.codes.p + r0 * ix->row_bytes, stream);
        MSVS_HIP(hipGetLastError());
        MSVS_HIP(hipMemcpyAsync(ch.list.data() + r0, d_assign.p, cnt * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream)); // d_x is reused by the next step
    }
    for (size_t i = 0; i < n; i++)
        if (ch.list[i] < 0 || (size_t)ch.list[i] >= ix->nlist)
            fail(MSVS_ERR_DEVICE, "internal: row %zu was assigned to list %d of %zu", i, ch.list[i], ix->nlist);
    ix->staged += n;
    ix->chunks.push_back(std::move(ch));
}

/// the final buffers of n rows: the codes in whole blocks of row_pad rows (at least one), zeroed where the index wants that
inline void alloc_lists(CodedIvf & ix, size_t n, size_t row_pad, bool zero_codes, hipStream_t stream)
{
    const size_t code_bytes = round_up(std::max<size_t>(n, 1), row_pad) * ix.row_bytes;
    ix.codes.alloc(code_bytes);
    if (zero_codes)
        MSVS_HIP(hipMemsetAsync(ix.codes.p, 0, code_bytes, stream)); // (the rows that fill the last block)
    ix.labels.alloc(std::max<size_t>(n, 1));
    ix.list_off.alloc(ix.nlist + 1);
}

/// labels and list offsets to the device, then the index is ready
inline void publish_lists(CodedIvf & ix, const std::vector<uint32_t> & h_labels, hipStream_t stream)
{
    if (ix.n)
        MSVS_HIP(hipMemcpyAsync(ix.labels.p, h_labels.data(), ix.n * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipMemcpyAsync(ix.list_off.p, ix.h_list_off.data(), (ix.nlist + 1) * 8, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
    ix.staged = ix.n;
    ix.ready = true;
}

/// msvs_*_index_build but for the scatter launch: scatter(src, dst, d_pos, cnt, stream) enqueues it for a staged chunk's
/// cnt rows
template <class Scatter>
inline void build_lists(CodedIvf * ix, const char * name, size_t row_pad, bool zero_codes, Scatter scatter)
{
    DeviceGuard on_device(ix ? ix->device : -1);
    check_index(ix);
    if (ix->ready)
        return;
    check_trained(*ix, name);
    hipStream_t stream = thread_stream();
    const size_t nlist = ix->nlist, n = ix->staged;
    std::vector<int32_t> list;
    std::vector<uint32_t> id;
    list.reserve(n);
    id.reserve(n);
    for (const auto & ch : ix->chunks)
        for (size_t i = 0; i < ch.n; i++)
        {
            list.push_back(ch.list[i]);
            id.push_back((uint32_t)ch.ids[i]);
        }
    ListLayout lay = list_major_layout(list.data(), id.data(), n, nlist);
    ix->h_list_off = std::move(lay.list_off);
    ix->max_list_len = lay.max_list_len;
    alloc_lists(*ix, n, row_pad, zero_codes, stream);
    std::vector<uint32_t> h_labels(n), pos(n); // pos: staged position -> list-major position
    for (size_t p = 0; p < n; p++)
    {
        h_labels[p] = id[lay.order[p]];
        pos[lay.order[p]] = (uint32_t)p;
    }
    size_t first = 0; // staged position of the chunk's first row
    for (size_t c = 0; c < ix->chunks.size(); first += ix->chunks[c].n, c++)
    {
        // a staged chunk goes to its list-major places and is released: staged + final codes never both whole beyond this point
        const size_t cnt = ix->chunks[c].n;
        DevBuf<uint32_t> d_pos(cnt);
        MSVS_HIP(hipMemcpyAsync(d_pos.p, pos.data() + first, cnt * 4, hipMemcpyHostToDevice, stream));
        scatter(ix->chunks[c].codes.p, ix->codes.p, d_pos.p, cnt, stream);
        MSVS_HIP(hipGetLastError());
        MSVS_HIP(hipStreamSynchronize(stream));
        ix->chunks[c].codes.release();
    }
    ix->chunks.clear();
    ix->n = n;
    publish_lists(*ix, h_labels, stream);
}

inline size_t coded_bytes(const CodedIvf & ix)
{
    size_t b = ix.codes.bytes() + ix.labels.bytes() + ix.list_off.bytes() + ix.centroids.bytes();
    for (const auto & ch : ix.chunks)
        b += ch.codes.bytes();
    return b;
}

// ------------------------------------------------------------------------------------------- search

/// one round of a search, as the scan sees it
struct ScanRound
{
    const float * dq;       // the round's queries, padded rows of ld floats
    const int32_t * probes; // their P lists each
    const GroupedPlan & plan;
    uint64_t * partial;
    const uint64_t * alive;
    size_t nbits, k, P, seg_max;
    uint32_t rpb;
    int metric; // M_L2 / M_IP
    // what an index asked for through RoundExtra (null otherwise)
    size_t nq = 0;                   // queries of the round
    const float * probe_dis = nullptr; // [query][probe] the canonical distance / inner product to every probe's centroid
    void * extra = nullptr;          // nq * RoundExtra::bytes_per_q bytes of the search's arena, 256-byte aligned
    // a later rank round of a search with k > MSVS_MAX_K (null otherwise): [query] the last key the query has returned; the scan
    // offers only rows whose key is strictly greater (its AFTER form)
    const uint64_t * after = nullptr;
};

/// What an index wants of a round beside the common buffers: scratch bytes per query of its own, the coarse step's distances.
struct RoundExtra
{
    size_t bytes_per_q = 0;
    bool probe_dis = false;
};

/// the fields every grouped scan's parameter block has
template <class Params>
inline void fill_scan_params(Params & a, const CodedIvf & ix, const ScanRound & r)
{
    a.labels = ix.labels.p;
    a.alive = r.alive;
    a.nbits = (uint32_t)std::min<size_t>(r.nbits, 0xffffffffu);
    a.partial = r.partial;
    a.k = (uint32_t)r.k;
    a.nprobe = (uint32_t)r.P;
    a.nlist = (uint32_t)ix.nlist;
    a.rows_per_block = r.rpb;
    a.seg_max = (uint32_t)r.seg_max;
    a.list_off = ix.list_off.p;
    a.pair_off = r.plan.pair_off;
    a.work_off = r.plan.work_off;
    a.pairs = r.plan.pairs;
    a.after = r.after;
}

/// Everything on the device, enqueued on `stream`: queries padded (and normalised for cosine) into scratch, the canonical coarse
/// quantiser over the centroids, the plan, the list scan over the codes, the per-query merge.  Row segments are whole steps of
/// row_step rows (rpb_knob: the index's option); pick_T(n_pairs, k) is the round's query tile, scan(T, grid, round) its launch.
/// extra: what the index wants beside (RoundExtra); prepare(round) enqueues its per-query work of a round, after the queries are
/// padded and normalised and before the plan (its round has no plan-dependent field to read: T, grid and the scan come later).
/// k_max: MSVS_MAX_K, or MSVS_MAX_K_ROUNDS for the entries that search in rank rounds.  k > MSVS_MAX_K: everything up to the plan
/// once per chunk of queries as ever, then ceil(k / MSVS_MAX_K) times the scan (k_round = min(MSVS_MAX_K, k - done) ranks, from the
/// second round on only rows whose key is strictly greater than the query's continuation key: ScanRound::after), the merge to keys
/// and launch_round_scatter.  All queries of the chunk advance together and nothing waits for the host: a query that has
/// finished rides through the later rounds admitting nothing.  Segments, tile, LDS and partial lists are sized by min(k, MSVS_MAX_K).
template <class PickT, class Prepare, class Scan>
inline void search_device(const CodedIvf & ix, const char * name, const char * prof_name, const float * d_queries, size_t nq, size_t k,
                          size_t k_max, size_t nprobe, const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream,
                          size_t row_step, double rpb_knob, RoundExtra extra, PickT pick_T, Prepare prepare, Scan scan)
{
    check_k(k, k_max);
    check_built(ix, name);
    if (nprobe < 1)
        fail(MSVS_ERR_INVALID_ARGUMENT, "nprobe must be >= 1");
    if (nq == 0 || k == 0)
        return;
    if (!d_queries || !d_ids || !d_dis)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    const size_t nlist = ix.nlist, P = std::min(nprobe, nlist);
    if (P > MSVS_MAX_K)
        fail(MSVS_ERR_UNSUPPORTED_K, "min(nprobe, nlist) = %zu exceeds the coarse quantiser's top-k limit %d", P, MSVS_MAX_K);
    const uint32_t ld = ix.ld;
    const int m = scan_metric(ix.metric);
    const bool rounds = k > MSVS_MAX_K;
    const size_t kl = std::min<size_t>(k, MSVS_MAX_K); // ranks of one scan
    // per query of a round: its padded row, its probes and pairs (rounds: a round's merged keys and the continuation key)
    const SegmentPlan sp = plan_segments(ix.max_list_len, rpb_knob, row_step, P, kl,
                                         (size_t)ld * 4 + P * 8 + 64 + extra.bytes_per_q + (extra.probe_dis ? P * 4 : 0)
                                             + (rounds ? (size_t)(MSVS_MAX_K + 1) * 8 : 0),
                                         nq);
    const uint32_t rpb = sp.rpb;
    const size_t seg_max = sp.seg_max, per_q = sp.per_q, chunk = sp.chunk;
    const size_t last = nq % chunk;
    const size_t coarse = std::max(flat_scratch_bytes(nlist, chunk, (uint32_t)P, ld), last ? flat_scratch_bytes(nlist, last, (uint32_t)P, ld) : 0);
    Scratch & scr = scratch_for(stream);
    scr.reserve(chunk * per_q + coarse + (nlist + 1) * 16 + 20 * 256, stream);
    float * dq = scr.take<float>(chunk * ld);
    int32_t * probes = scr.take<int32_t>(chunk * P);
    float * probe_dis = extra.probe_dis ? scr.take<float>(chunk * P) : nullptr;
    void * extra_buf = extra.bytes_per_q ? scr.take<unsigned char>(chunk * extra.bytes_per_q) : nullptr;
    const GroupedPlan plan(scr, nlist, chunk * P);
    uint64_t * partial = scr.take<uint64_t>(chunk * P * seg_max * kl);
    uint64_t * round_keys = rounds ? scr.take<uint64_t>(chunk * MSVS_MAX_K) : nullptr;
    uint64_t * after = rounds ? scr.take<uint64_t>(chunk) : nullptr;
    const size_t mark = scr.used;
    for (size_t q0 = 0; q0 < nq; q0 += chunk)
    {
        const size_t nqc = std::min(chunk, nq - q0);
        upload_rows(dq, d_queries + q0 * ix.dim, nqc, (uint32_t)ix.dim, ld, MSVS_MEM_DEVICE, stream);
        if (ix.metric == MSVS_METRIC_COSINE)
            normalize_device_rows(dq, nqc, (uint32_t)ix.dim, ld, stream);
        // 1. the canonical exact top-P of the centroids, ordered by (distance, list id)
        scr.used = mark;
        MergeParams co{};
        co.mode = 1;
        co.out_probes = probes;
        co.out_probe_dis = probe_dis;
        flat_search_device(scr, m, ix.centroids.p, nullptr, nlist, ld, dq, nqc, (uint32_t)P, nullptr, 0, co, stream);
        const ScanRound first{dq, probes, plan, partial, d_alive, nbits, kl, P, seg_max, rpb, m, nqc, probe_dis, extra_buf};
        prepare(first);
        MSVS_HIP(hipGetLastError());
        // 2. (query, list) pairs grouped by list -> (list, query tile, row segment) items
        const size_t n_pairs = nqc * P;
        const uint32_t T = pick_T(n_pairs, kl);
        plan.run(probes, ix.list_off.p, n_pairs, rpb, T, stream);
        for (size_t done = 0; done < k; done += MSVS_MAX_K) // (one pass unless `rounds`)
        {
            const size_t kr = std::min<size_t>(MSVS_MAX_K, k - done);
            const ScanRound round{dq, probes, plan, partial, d_alive, nbits, kr, P, seg_max, rpb, m, nqc, probe_dis, extra_buf, done ? after : nullptr};
            // 3. the list scan over the codes
            {
                ProfileScope prof(prof_name, stream);
                const uint32_t grid = (uint32_t)std::min<size_t>(2048, n_pairs * seg_max);
                scan(T, grid, round);
                MSVS_HIP(hipGetLastError());
            }
            // 4. per-query top-k over the valid segments of its probed lists
            IvfMergeParams im{};
            im.partial = partial;
            im.probes = probes;
            im.list_off = ix.list_off.p;
            im.nprobe = (uint32_t)P;
            im.seg_max = (uint32_t)seg_max;
            im.rows_per_block = rpb;
            im.k = (uint32_t)kr;
            im.out_ids = d_ids + q0 * k;
            im.out_dis = d_dis + q0 * k;
            im.cosine = ix.metric == MSVS_METRIC_COSINE;
            im.out_keys = round_keys;
            launch_ivf_merge(m, im, (uint32_t)nqc, stream);
            if (rounds)
                launch_round_scatter(m, round_keys, nqc, kr, k, done, ix.metric == MSVS_METRIC_COSINE, d_ids + q0 * k, d_dis + q0 * k, after, stream);
        }
    }
}

/// ... for an index that wants nothing beside
template <class PickT, class Scan>
inline void search_device(const CodedIvf & ix, const char * name, const char * prof_name, const float * d_queries, size_t nq, size_t k,
                          size_t k_max, size_t nprobe, const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream,
                          size_t row_step, double rpb_knob, PickT pick_T, Scan scan)
{
    search_device(ix, name, prof_name, d_queries, nq, k, k_max, nprobe, d_alive, nbits, d_ids, d_dis, stream, row_step, rpb_knob, RoundExtra{}, pick_T,
                  [](const ScanRound &) {}, scan);
}

/// The host-pointer entry: queries and filter staged to the device, dev(d_queries, nprobe, d_alive, d_ids, d_dis, stream) is the
/// index's device search, results copied back; synchronises.  k_max: the entry's limit of k.
template <class DeviceSearch>
inline void search_host(const CodedIvf * ix, const char * name, const float * queries, size_t nq, size_t k, size_t k_max, const char * params,
                        const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis, DeviceSearch dev)
{
    DeviceGuard on_device(ix ? ix->device : -1);
    check_index(ix);
    const size_t nprobe = parse_nprobe(params);
    check_k(k, k_max);
    check_built(*ix, name);
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
    dev(dq, nprobe, d_alive, d_ids, d_dis, stream);
    MSVS_HIP(hipMemcpyAsync(ids, d_ids, nq * k * 8, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipMemcpyAsync(dis, d_dis, nq * k * 4, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------------------------------------- two-stage search

/// msvs_refine_device (refine.hip): the candidates' labels scored against the row store's f32 rows, the best k; enqueued on `stream`
void refine_device(const msvs_rows * rows, int metric, const float * d_queries, size_t nq, const int64_t * d_cand, size_t kc, size_t k,
                   int64_t * d_ids, float * d_dis, hipStream_t stream);

/// The composed entries: first(d_cand_ids, d_cand_dis) is the index's own device search with kc results (the filter applies
/// there), its labels stay in an arena of their own on the same stream, then the refine step with the index's metric: no host round trip between.
/// kc_max: MSVS_MAX_K, or MSVS_REFINE_MAX_CAND for the entries whose first stage searches in rank rounds.
template <class FirstStage>
inline void search_refine_device(const CodedIvf & ix, const char * name, const msvs_rows * rows, const float * d_queries, size_t nq, size_t k,
                                 size_t kc, size_t kc_max, int64_t * d_ids, float * d_dis, hipStream_t stream, FirstStage first)
{
    if (!rows)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null row store");
    if (msvs_rows_dim(rows) != ix.dim || (msvs_rows_normalized(rows) != 0) != (ix.metric == MSVS_METRIC_COSINE))
        fail(MSVS_ERR_INVALID_ARGUMENT, "the row store (dim %zu, normalize=%d) does not fit the %s index (dim %zu, %s)", msvs_rows_dim(rows),
             msvs_rows_normalized(rows), name, ix.dim, ix.metric == MSVS_METRIC_COSINE ? "cosine: normalize=1" : "L2 / IP: normalize=0");
    check_k(kc, kc_max);
    if (k > kc)
        fail(MSVS_ERR_INVALID_ARGUMENT, "k = %zu exceeds kc = %zu, the first stage's results", k, kc);
    check_k(k); // (kc_max > MSVS_MAX_K: the refine step's own limit)
    check_built(ix, name);
    if (nq == 0 || k == 0)
        return;
    if (!d_queries || !d_ids || !d_dis)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    Scratch & aux = aux_for(stream); // (the first stage and the refine step both take scratch_for)
    aux.reserve(nq * kc * 12 + 2 * 256, stream);
    int64_t * c_ids = aux.take<int64_t>(nq * kc);
    float * c_dis = aux.take<float>(nq * kc);
    first(c_ids, c_dis);
    refine_device(rows, ix.metric, d_queries, nq, c_ids, kc, k, d_ids, d_dis, stream);
}

// ------------------------------------------------------------------------------------------- export and files

/// the built index's labels, on the host
inline void fetch_labels(const CodedIvf & ix, int64_t * ids, hipStream_t stream)
{
    if (!ids || !ix.n)
        return;
    std::vector<uint32_t> l32(ix.n);
    MSVS_HIP(hipMemcpyAsync(l32.data(), ix.labels.p, ix.n * 4, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    for (size_t i = 0; i < ix.n; i++)
        ids[i] = (int64_t)l32[i];
}

/// export's head: the codebook must exist; the centroids
inline void export_head(const CodedIvf * ix, const char * name, float * centroids)
{
    check_index(ix);
    check_trained(*ix, name);
    if (centroids)
        memcpy(centroids, ix->h_cent.data(), ix->h_cent.size() * 4);
}

/// export's list part: false if the caller asked for none of it; else the index must be built; the list offsets
inline bool export_lists(const CodedIvf & ix, const char * name, int64_t * list_off, const uint8_t * codes, const int64_t * ids)
{
    if (!list_off && !codes && !ids)
        return false;
    if (!ix.ready)
        fail(MSVS_ERR_NOT_READY, "the %s index is not built: it has no lists to export", name);
    if (list_off)
        memcpy(list_off, ix.h_list_off.data(), (ix.nlist + 1) * 8);
    return true;
}

struct IdHeader // 24 bytes, little endian
{
    char magic[8]; // "MSVSSQID" / "MSVSPQID"
    uint64_t n;
    uint64_t check; // FNV-1a of the bytes before it
};

inline void write_id_file(const msvs_io_t * io, const char * file, const char * magic, const std::vector<int64_t> & ids)
{
    IoStream f(io, file, 1);
    IdHeader h{};
    memcpy(h.magic, magic, 8);
    h.n = ids.size();
    h.check = fnv1a(&h, offsetof(IdHeader, check));
    f.write(&h, sizeof(h));
    if (!ids.empty())
        f.write(ids.data(), ids.size() * 8);
    f.finish();
}

inline std::vector<int64_t> read_id_file(const msvs_io_t * io, const char * file, const char * magic, size_t n, const char * name)
{
    std::vector<int64_t> ids;
    IoStream f(io, file, 0);
    IdHeader h{};
    f.read(&h, sizeof(h));
    if (memcmp(h.magic, magic, 8) != 0 || h.check != fnv1a(&h, offsetof(IdHeader, check)) || h.n != n)
        fail(MSVS_ERR_IO, "corrupt msvs %s id list header", name);
    read_grow(f, ids, n);
    expect_end(f);
    for (int64_t id : ids)
        if (id < 0 || id >= (int64_t)CODED_LABEL_END)
            fail(MSVS_ERR_IO, "corrupt msvs %s id list: label %lld outside [0, 2^32 - 1)", name, (long long)id);
    return ids;
}

/// the list offsets of a data file (ix.nlist and ix.n are set): read, checked, the longest list noted
inline void read_list_offsets(IoStream & f, CodedIvf & ix, const char * name)
{
    read_grow(f, ix.h_list_off, ix.nlist + 1);
    const std::string bad = list_offsets_error(ix.h_list_off, ix.n, (std::string("msvs ") + name + " index").c_str());
    if (!bad.empty())
        fail(MSVS_ERR_IO, "%s", bad.c_str());
    ix.max_list_len = longest_list(ix.h_list_off);
}

/// the tail of a load: the labels as u32 and the list offsets to the device, then the index is ready
inline void finish_load(CodedIvf & ix, const std::vector<int64_t> & ids, hipStream_t stream)
{
    std::vector<uint32_t> l32(ix.n);
    for (size_t i = 0; i < ix.n; i++)
        l32[i] = (uint32_t)ids[i];
    publish_lists(ix, l32, stream);
}
}
