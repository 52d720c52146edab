// pq_index.hip -- the IVFPQ index (include/msvs.h: msvs_pq_index_*): coarse centroids + m sub-quantisers of 256 entries over the
// residuals; codes, lists and labels are all the index keeps.  Semantics and layout: pq_ivf_kernels.hpp, DESIGN.md 4.12.
// Reused as they are: the k-means trainer (temporary IVFFLAT indexes, for the coarse centroids and for every sub-codebook), the
// assignment kernel, flat_search_device for the coarse step, GroupedPlan, plan_segments, launch_ivf_merge, Scratch,
// normalize_device_rows, upload_rows.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "index_internal.hpp"
#include "io_stream.hpp"
#include "ivf_build_kernels.hpp"
#include "list_layout.hpp"
#include "pq_ivf_kernels.hpp"

using namespace msvs;

namespace
{
constexpr size_t PQ_ADD_ROWS = 65536;          // rows of a chunk on the device as f32 at a time (encode, residuals)
constexpr size_t PQ_TRAIN_ROWS = 262144;       // residuals the sub-codebooks are trained on at most
constexpr size_t PQ_KSUB = 256;                // entries of a sub-codebook (8 bits)
constexpr uint32_t PQ_LABEL_END = 0xffffffffu; // labels are < this

/// dim / m of an index that can exist: the smallest tile with the largest k must fit the scan's LDS
inline bool pq_fits(size_t dim, size_t m)
{
    return dim >= 1 && dim <= 8192 && m >= 1 && m <= 128 && dim % m == 0
        && pq_lds_bytes(1, (uint32_t)m, padded_dim(dim), MSVS_MAX_K) <= PQ_LDS_BUDGET;
}
}

struct msvs_pq_index
{
    int metric = MSVS_METRIC_L2;
    size_t dim = 0, m = 0, dsub = 0;
    uint32_t ld = 0; // round_up(dim, 4): floats per centroid / query row
    uint32_t mw = 0; // 32-bit words of a stored row: ceil(m / 4)
    int device = 0;
    std::string params; // create's, handed to the temporary IVFFLAT indexes that run the k-means
    // codebook
    size_t nlist = 0;
    DevBuf<float> centroids;   // nlist x ld
    std::vector<float> h_cent; // nlist x dim
    std::vector<float> h_cb;   // [m][256][dsub]
    DevBuf<float> cbT;         // [m][dsub][256]
    bool trained = false;
    // staging (between add and build): codes, list and label only
    struct Chunk
    {
        DevBuf<uint32_t> codes; // n x mw, row-major
        std::vector<int32_t> list;
        std::vector<int64_t> ids;
        size_t n = 0;
    };
    std::vector<Chunk> chunks;
    size_t staged = 0;
    // final storage
    DevBuf<uint32_t> codes;   // round_up(n, 64) x mw, list-major, blocks of 64 rows transposed (pq_code_word)
    DevBuf<uint32_t> labels;  // n
    DevBuf<int64_t> list_off; // nlist + 1
    std::vector<int64_t> h_list_off;
    size_t n = 0, max_list_len = 0;
    bool ready = false;
};

static void pq_set_geometry(msvs_pq_index & ix, int metric, size_t dim, size_t m)
{
    ix.metric = metric;
    ix.dim = dim;
    ix.m = m;
    ix.dsub = dim / m;
    ix.ld = padded_dim(dim);
    ix.mw = (uint32_t)ceil_div(m, (size_t)4);
}

/// centroids (nlist x ld on the device already) + sub-codebooks [m][256][dsub] on the host -> the index's codebook
static void pq_set_codebooks(msvs_pq_index & ix, const float * cb, hipStream_t stream)
{
    const size_t d = ix.dim, m = ix.m, dsub = ix.dsub;
    for (size_t i = 0; i < PQ_KSUB * d; i++)
        if (!std::isfinite(cb[i]))
            fail(MSVS_ERR_INVALID_ARGUMENT, "codebook entry %zu of sub-quantiser %zu is not finite", (i / dsub) % PQ_KSUB, i / (PQ_KSUB * dsub));
    ix.h_cb.assign(cb, cb + PQ_KSUB * d);
    std::vector<float> t(PQ_KSUB * d);
    for (size_t s = 0; s < m; s++)
        for (size_t j = 0; j < PQ_KSUB; j++)
            for (size_t u = 0; u < dsub; u++)
                t[(s * dsub + u) * PQ_KSUB + j] = cb[(s * PQ_KSUB + j) * dsub + u];
    ix.cbT.alloc(PQ_KSUB * d);
    MSVS_HIP(hipMemcpyAsync(ix.cbT.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, stream));
    ix.h_cent.resize(ix.nlist * d);
    MSVS_HIP(hipMemcpy2DAsync(ix.h_cent.data(), d * 4, ix.centroids.p, (size_t)ix.ld * 4, d * 4, ix.nlist, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream)); // t is about to go
    ix.trained = true;
}

static void pq_drop_codebook(msvs_pq_index & ix)
{
    ix.trained = false;
    ix.nlist = 0;
    ix.centroids.release();
    ix.cbT.release();
    ix.h_cent.clear();
    ix.h_cb.clear();
}

/// nearest centroid of n device rows (stride ld): by L2 for L2 indexes, by inner product for IP and cosine (as msvs_index_add)
static void pq_assign(const msvs_pq_index & ix, const float * d_x, size_t n, int32_t * d_assign, float * d_cnorm, hipStream_t stream)
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

/// cnt dense rows (host or device) -> stored rows on the device (padded, normalised for cosine) and their lists
static void pq_stage_rows(const msvs_pq_index & ix, const float * x, size_t cnt, int mem, float * d_x, int32_t * d_assign, float * d_cnorm,
                          hipStream_t stream)
{
    upload_rows(d_x, x, cnt, (uint32_t)ix.dim, ix.ld, mem, stream);
    if (ix.metric == MSVS_METRIC_COSINE)
        normalize_device_rows(d_x, cnt, (uint32_t)ix.dim, ix.ld, stream);
    pq_assign(ix, d_x, cnt, d_assign, d_cnorm, stream);
}

static void pq_check_codebook_time(const msvs_pq_index * ix)
{
    if (ix->staged || ix->ready)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the codebook must be set before data is added");
}

/// a temporary IVFFLAT index trained on (x, n): the k-means as it is.  The caller frees it.
static msvs_index_t * pq_kmeans(int metric, size_t dim, const std::string & params, const float * x, size_t n, int mem)
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
    return tmp;
}

extern "C" int msvs_pq_index_create(int metric, size_t dim, const char * params, msvs_pq_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        *out = nullptr;
        if (metric != MSVS_METRIC_L2 && metric != MSVS_METRIC_IP && metric != MSVS_METRIC_COSINE)
            fail(MSVS_ERR_NOT_IMPLEMENTED, "metric %d is not implemented for the IVFPQ index", metric);
        auto p = parse_params(params);
        if (param_int(p, "ncentroids", 1024) < 1)
            fail(MSVS_ERR_INVALID_ARGUMENT, "bad ncentroids");
        const long m = param_int(p, "m", 0);
        if (m < 1 || !pq_fits(dim, (size_t)m))
            fail(MSVS_ERR_INVALID_ARGUMENT,
                 "the IVFPQ index needs 1 <= m <= 128 dividing 1 <= dim <= 8192 and tables of m KiB + 8 * dim + 10 KiB within 160 KiB (dim %zu, m %ld)",
                 dim, m);
        std::unique_ptr<msvs_pq_index> ix(new msvs_pq_index);
        pq_set_geometry(*ix, metric, dim, (size_t)m);
        ix->params = params ? params : "";
        MSVS_HIP(hipGetDevice(&ix->device));
        *out = ix.release();
    });
}

extern "C" void msvs_pq_index_free(msvs_pq_index_t * ix) { delete ix; }

extern "C" int msvs_pq_index_set_codebook(msvs_pq_index_t * ix, const float * centroids, size_t nlist, const float * codebooks, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || !centroids || !codebooks || nlist == 0 || nlist > 0x7fffffffull)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / codebook");
        pq_check_codebook_time(ix);
        hipStream_t stream = thread_stream();
        std::vector<float> cb(PQ_KSUB * ix->dim);
        if (mem == MSVS_MEM_DEVICE)
            MSVS_HIP(hipMemcpyAsync(cb.data(), codebooks, cb.size() * 4, hipMemcpyDeviceToHost, stream));
        else
            memcpy(cb.data(), codebooks, cb.size() * 4);
        pq_drop_codebook(*ix);
        ix->centroids.alloc(nlist * ix->ld);
        upload_rows(ix->centroids.p, centroids, nlist, (uint32_t)ix->dim, ix->ld, mem, stream);
        MSVS_HIP(hipStreamSynchronize(stream));
        ix->nlist = nlist;
        try
        {
            pq_set_codebooks(*ix, cb.data(), stream);
        }
        catch (...)
        {
            pq_drop_codebook(*ix); // a refused codebook leaves none
            throw;
        }
    });
}

extern "C" int msvs_pq_index_train(msvs_pq_index_t * ix, const float * x, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || (n && !x))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / data");
        pq_check_codebook_time(ix);
        if (n < PQ_KSUB)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the IVFPQ index needs at least 256 training rows (%zu given)", n);
        hipStream_t stream = thread_stream();
        const size_t d = ix->dim, m = ix->m, dsub = ix->dsub;
        pq_drop_codebook(*ix);
        {
            // the coarse centroids: the IVFFLAT trainer as it is, through a temporary index of the same metric and parameters
            std::unique_ptr<msvs_index_t, void (*)(msvs_index_t *)> tmp(pq_kmeans(ix->metric, d, ix->params, x, n, mem), msvs_index_free);
            ix->nlist = tmp->nlist;
            ix->centroids.alloc(ix->nlist * ix->ld);
            MSVS_HIP(hipMemsetAsync(ix->centroids.p, 0, ix->nlist * ix->ld * 4, stream));
            MSVS_HIP(hipMemcpy2DAsync(ix->centroids.p, (size_t)ix->ld * 4, tmp->centroids.p, (size_t)tmp->ld * 4, d * 4, ix->nlist,
                                      hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        // the residuals fl(x - c_l) of the evenly spaced training rows floor(i * n / cap), dense on the device
        const size_t cap = std::min(n, PQ_TRAIN_ROWS);
        DevBuf<float> d_res(cap * d);
        {
            const size_t step_rows = std::min(cap, PQ_ADD_ROWS);
            DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist), d_pick(mem == MSVS_MEM_DEVICE && cap < n ? step_rows * d : 0);
            DevBuf<int32_t> d_assign(step_rows);
            std::vector<float> h_pick(mem != MSVS_MEM_DEVICE && cap < n ? step_rows * d : 0);
            for (size_t i0 = 0; i0 < cap; i0 += step_rows)
            {
                const size_t cnt = std::min(step_rows, cap - i0);
                const float * src = x + i0 * d; // cap == n: the rows themselves
                int src_mem = mem;
                if (cap < n && mem == MSVS_MEM_DEVICE)
                {
                    hipLaunchKernelGGL(pq_pick_rows_kernel, dim3((unsigned)ceil_div(cnt * d, (size_t)256)), dim3(256), 0, stream, x, n, cap, i0, cnt,
                                       (uint32_t)d, d_pick.p);
                    MSVS_HIP(hipGetLastError());
                    src = d_pick.p;
                }
                else if (cap < n)
                {
                    for (size_t i = 0; i < cnt; i++)
                        memcpy(&h_pick[i * d], x + ((i0 + i) * n / cap) * d, d * 4);
                    src = h_pick.data();
                    src_mem = MSVS_MEM_HOST;
                }
                pq_stage_rows(*ix, src, cnt, src_mem, d_x.p, d_assign.p, d_cnorm.p, stream);
                hipLaunchKernelGGL(pq_residual_kernel, dim3((unsigned)ceil_div(cnt * d, (size_t)256)), dim3(256), 0, stream, d_x.p, d_assign.p,
                                   ix->centroids.p, cnt, (uint32_t)d, ix->ld, d_res.p + i0 * d);
                MSVS_HIP(hipGetLastError());
                MSVS_HIP(hipStreamSynchronize(stream)); // d_x / h_pick are reused by the next step
            }
        }
        // every sub-codebook: the same trainer over the sub-space's columns, L2, 256 centroids, the caller's iterations and seed
        std::string sub_params;
        for (const auto & kv : parse_params(ix->params.c_str()))
            if (kv.first != "ncentroids" && kv.first != "m")
                sub_params += kv.first + "=" + kv.second + ",";
        sub_params += "ncentroids=256";
        DevBuf<float> d_sub(cap * dsub);
        std::vector<float> cb(PQ_KSUB * d);
        for (size_t s = 0; s < m; s++)
        {
            MSVS_HIP(hipMemcpy2DAsync(d_sub.p, dsub * 4, d_res.p + s * dsub, d * 4, dsub * 4, cap, hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
            std::unique_ptr<msvs_index_t, void (*)(msvs_index_t *)> tmp(pq_kmeans(MSVS_METRIC_L2, dsub, sub_params, d_sub.p, cap, MSVS_MEM_DEVICE),
                                                                        msvs_index_free);
            if (tmp->nlist != PQ_KSUB)
                fail(MSVS_ERR_DEVICE, "internal: sub-quantiser %zu came out with %zu centroids", s, tmp->nlist);
            MSVS_HIP(hipMemcpy2D(cb.data() + s * PQ_KSUB * dsub, dsub * 4, tmp->centroids.p, (size_t)tmp->ld * 4, dsub * 4, PQ_KSUB,
                                 hipMemcpyDeviceToHost));
        }
        try
        {
            pq_set_codebooks(*ix, cb.data(), stream);
        }
        catch (...)
        {
            pq_drop_codebook(*ix);
            throw;
        }
    });
}

extern "C" int msvs_pq_index_add(msvs_pq_index_t * ix, const float * x, const int64_t * ids, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || (n && !x))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / data");
        if (ix->ready)
            fail(MSVS_ERR_INVALID_ARGUMENT, "index already built");
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index has no codebook yet (train / set_codebook)");
        if (n == 0)
            return;
        if (ix->staged + n > 0xfffffff0ull)
            fail(MSVS_ERR_ID_RANGE, "more rows than the u32 row range");
        hipStream_t stream = thread_stream();
        msvs_pq_index::Chunk ch;
        ch.n = n;
        ch.ids.resize(n);
        if (ids)
        {
            if (mem == MSVS_MEM_DEVICE)
                MSVS_HIP(hipMemcpy(ch.ids.data(), ids, n * 8, hipMemcpyDeviceToHost));
            else
                memcpy(ch.ids.data(), ids, n * 8);
        }
        else
            for (size_t i = 0; i < n; i++)
                ch.ids[i] = (int64_t)(ix->staged + i);
        for (size_t i = 0; i < n; i++)
            if (ch.ids[i] < 0 || ch.ids[i] >= (int64_t)PQ_LABEL_END)
                fail(MSVS_ERR_ID_RANGE, "id %lld is outside the label range [0, 2^32 - 1)", (long long)ch.ids[i]);
        const uint32_t mw = ix->mw;
        ch.codes.alloc(n * mw);
        MSVS_HIP(hipMemsetAsync(ch.codes.p, 0, n * mw * 4, stream)); // the padding bytes of a row are 0
        ch.list.resize(n);
        // the encoder stages a row and its centroid in LDS: more than 64 KiB of it (dim > 8184, beside its 64 static bytes) needs the
        // attribute raised once
        static std::once_flag once;
        std::call_once(once, [] {
            MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         2 * 8192 * 4));
        });
        const size_t step_rows = std::min(n, PQ_ADD_ROWS);
        DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist);
        DevBuf<int32_t> d_assign(step_rows);
        for (size_t r0 = 0; r0 < n; r0 += step_rows)
        {
            const size_t cnt = std::min(step_rows, n - r0);
            pq_stage_rows(*ix, x + r0 * ix->dim, cnt, mem, d_x.p, d_assign.p, d_cnorm.p, stream);
            const uint32_t rpb = 8;
            hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)ceil_div(cnt, (size_t)rpb)), dim3(BLOCK), 2 * ix->dim * 4, stream, d_x.p, d_assign.p,
                               ix->centroids.p, ix->cbT.p, cnt, (uint32_t)ix->dim, ix->ld, (uint32_t)ix->m, (uint32_t)ix->dsub, mw * 4, rpb,
                               reinterpret_cast<uint8_t *>(ch.codes.p + r0 * mw));
            MSVS_HIP(hipGetLastError());
            MSVS_HIP(hipMemcpyAsync(ch.list.data() + r0, d_assign.p, cnt * 4, hipMemcpyDeviceToHost, stream));
            MSVS_HIP(hipStreamSynchronize(stream)); // d_x is reused by the next step
        }
        for (size_t i = 0; i < n; i++)
            if (ch.list[i] < 0 || (size_t)ch.list[i] >= ix->nlist)
                fail(MSVS_ERR_DEVICE, "internal: row %zu was assigned to list %d of %zu", i, ch.list[i], ix->nlist);
        ix->staged += n;
        ix->chunks.push_back(std::move(ch));
    });
}

extern "C" int msvs_pq_index_build(msvs_pq_index_t * ix)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (ix->ready)
            return;
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index has no codebook yet (train / set_codebook)");
        hipStream_t stream = thread_stream();
        const size_t nlist = ix->nlist, n = ix->staged;
        const uint32_t mw = ix->mw;
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
        const size_t code_words = std::max<size_t>(round_up(n, 64), 64) * mw;
        ix->codes.alloc(code_words);
        MSVS_HIP(hipMemsetAsync(ix->codes.p, 0, code_words * 4, stream)); // (the rows that fill the last block of 64)
        ix->labels.alloc(std::max<size_t>(n, 1));
        ix->list_off.alloc(nlist + 1);
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
            hipLaunchKernelGGL(pq_scatter_rows_kernel, dim3((unsigned)ceil_div(cnt * mw, (size_t)256)), dim3(256), 0, stream, ix->chunks[c].codes.p,
                               ix->codes.p, d_pos.p, cnt, mw);
            MSVS_HIP(hipGetLastError());
            MSVS_HIP(hipStreamSynchronize(stream));
            ix->chunks[c].codes.release();
        }
        if (n)
            MSVS_HIP(hipMemcpyAsync(ix->labels.p, h_labels.data(), n * 4, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipMemcpyAsync(ix->list_off.p, ix->h_list_off.data(), (nlist + 1) * 8, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        ix->chunks.clear();
        ix->n = n;
        MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
        ix->ready = true;
    });
}

extern "C" int msvs_pq_index_ready(const msvs_pq_index_t * ix) { return ix && ix->ready ? 1 : 0; }
extern "C" size_t msvs_pq_index_num_data(const msvs_pq_index_t * ix) { return ix ? (ix->ready ? ix->n : ix->staged) : 0; }
extern "C" size_t msvs_pq_index_num_lists(const msvs_pq_index_t * ix) { return ix ? ix->nlist : 0; }
extern "C" size_t msvs_pq_index_memory_usage(const msvs_pq_index_t * ix)
{
    if (!ix)
        return 0;
    size_t b = ix->codes.bytes() + ix->labels.bytes() + ix->list_off.bytes() + ix->centroids.bytes() + ix->cbT.bytes();
    for (const auto & ch : ix->chunks)
        b += ch.codes.bytes();
    return b;
}

// ------------------------------------------------------------------------------------------- search

template <int METRIC, int T, int R>
static void pq_launch(uint32_t grid, size_t lds, const PqIvfParams & a, hipStream_t stream)
{
    // more than 64 KiB of dynamic LDS needs the attribute raised once per kernel
    static std::once_flag once;
    std::call_once(once, [] {
        const void * fn = reinterpret_cast<const void *>(&pq_ivf_scan_kernel<METRIC, T, R>);
        hipFuncAttributes fa{};
        MSVS_HIP(hipFuncGetAttributes(&fa, fn));
        if (fa.sharedSizeBytes != 0) // PQ_LDS_BUDGET: the dynamic image may be the whole LDS
            fail(MSVS_ERR_DEVICE, "the IVFPQ list scan has %zu bytes of static LDS: pq_fits no longer holds", (size_t)fa.sharedSizeBytes);
        MSVS_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQ_LDS_BUDGET));
    });
    hipLaunchKernelGGL((pq_ivf_scan_kernel<METRIC, T, R>), dim3(grid), dim3(BLOCK), lds, stream, a);
}

template <int METRIC, int T>
static void pq_dispatch_r(uint32_t grid, size_t lds, const PqIvfParams & a, hipStream_t stream)
{
    switch (r_for_k(a.k))
    {
        case 1: pq_launch<METRIC, T, 1>(grid, lds, a, stream); break;
        case 2: pq_launch<METRIC, T, 2>(grid, lds, a, stream); break;
        default: pq_launch<METRIC, T, 4>(grid, lds, a, stream); break;
    }
}

template <int METRIC>
static void pq_dispatch_t(uint32_t T, uint32_t grid, const PqIvfParams & a, hipStream_t stream)
{
    const size_t lds = pq_lds_bytes(T, a.m, a.ld, a.k);
    switch (T)
    {
        case 1: pq_dispatch_r<METRIC, 1>(grid, lds, a, stream); break;
        case 2: pq_dispatch_r<METRIC, 2>(grid, lds, a, stream); break;
        case 4: pq_dispatch_r<METRIC, 4>(grid, lds, a, stream); break;
        default: pq_dispatch_r<METRIC, 8>(grid, lds, a, stream); break;
    }
}

/// Everything on the device, enqueued on `stream`: queries padded (and normalised for cosine) into scratch, the canonical coarse
/// quantiser over the centroids, the plan, the table-building list scan over the codes, the per-query merge.
static void pq_search_device(const msvs_pq_index & ix, const float * d_queries, size_t nq, size_t k, size_t nprobe, const uint64_t * d_alive,
                             size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    check_k(k);
    if (!ix.ready)
        fail(MSVS_ERR_NOT_READY, "the IVFPQ index is not built");
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
    const int metric = scan_metric(ix.metric);
    // row segments of whole 256-row steps (a segment rebuilds its tile's tables); per query of a round: its padded row, its probes and pairs
    const SegmentPlan sp = plan_segments(ix.max_list_len, options().pq_ivf_rpb, BLOCK, P, k, (size_t)ld * 4 + P * 8 + 64, nq);
    const uint32_t rpb = sp.rpb;
    const size_t seg_max = sp.seg_max, per_q = sp.per_q, chunk = sp.chunk;
    const size_t last = nq % chunk;
    const size_t coarse = std::max(flat_scratch_bytes(nlist, chunk, (uint32_t)P, ld), last ? flat_scratch_bytes(nlist, last, (uint32_t)P, ld) : 0);
    Scratch & scr = scratch_for(stream);
    scr.reserve(chunk * per_q + coarse + (nlist + 1) * 16 + 16 * 256, stream);
    float * dq = scr.take<float>(chunk * ld);
    int32_t * probes = scr.take<int32_t>(chunk * P);
    const GroupedPlan plan(scr, nlist, chunk * P);
    uint64_t * partial = scr.take<uint64_t>(chunk * P * seg_max * k);
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
        flat_search_device(scr, metric, ix.centroids.p, nullptr, nlist, ld, dq, nqc, (uint32_t)P, nullptr, 0, co, stream);
        // 2. (query, list) pairs grouped by list -> (list, query tile, row segment) items; the tile by the pairs per list, halved until
        //    its tables fit
        const size_t n_pairs = nqc * P;
        uint32_t T = n_pairs >= 16 * nlist ? 8 : (n_pairs >= 2 * nlist ? 4 : (n_pairs >= nlist ? 2 : 1));
        while (T > 1 && pq_lds_bytes(T, (uint32_t)ix.m, ld, (uint32_t)k) > PQ_LDS_BUDGET)
            T /= 2;
        plan.run(probes, ix.list_off.p, n_pairs, rpb, T, stream);
        // 3. the list scan over the codes
        PqIvfParams a{};
        a.codes = ix.codes.p;
        a.labels = ix.labels.p;
        a.alive = d_alive;
        a.nbits = (uint32_t)std::min<size_t>(nbits, 0xffffffffu);
        a.Q = dq;
        a.cent = ix.centroids.p;
        a.cbT = ix.cbT.p;
        a.partial = partial;
        a.ld = ld;
        a.dim = (uint32_t)ix.dim;
        a.m = (uint32_t)ix.m;
        a.dsub = (uint32_t)ix.dsub;
        a.mw = ix.mw;
        a.k = (uint32_t)k;
        a.nprobe = (uint32_t)P;
        a.nlist = (uint32_t)nlist;
        a.rows_per_block = rpb;
        a.seg_max = (uint32_t)seg_max;
        a.tables_only = options().pq_ivf_tables_only != 0;
        a.list_off = ix.list_off.p;
        a.pair_off = plan.pair_off;
        a.work_off = plan.work_off;
        a.pairs = plan.pairs;
        {
            ProfileScope prof("pq_ivf_scan", stream);
            const uint32_t grid = (uint32_t)std::min<size_t>(2048, n_pairs * seg_max);
            if (metric == M_IP)
                pq_dispatch_t<M_IP>(T, grid, a, stream);
            else
                pq_dispatch_t<M_L2>(T, grid, a, stream);
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
        im.k = (uint32_t)k;
        im.out_ids = d_ids + q0 * k;
        im.out_dis = d_dis + q0 * k;
        im.cosine = ix.metric == MSVS_METRIC_COSINE;
        launch_ivf_merge(metric, im, (uint32_t)nqc, stream);
    }
}

extern "C" int msvs_pq_index_search_device(const msvs_pq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                           const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] {
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        pq_search_device(*ix, d_queries, nq, k, nprobe, d_alive_bits, nbits, d_ids, d_dis, as_stream(hip_stream));
    });
}

extern "C" int msvs_pq_index_search(const msvs_pq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                    const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        const size_t nprobe = parse_nprobe(params);
        check_k(k);
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index is not built");
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
        pq_search_device(*ix, dq, nq, k, nprobe, d_alive, nbits, d_ids, d_dis, stream);
        MSVS_HIP(hipMemcpyAsync(ids, d_ids, nq * k * 8, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipMemcpyAsync(dis, d_dis, nq * k * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
    });
}

// ------------------------------------------------------------------------------------------- export and files

/// the built index's codes in NATURAL order (n x m) and its labels, on the host
static void pq_fetch(const msvs_pq_index & ix, uint8_t * codes, int64_t * ids, hipStream_t stream)
{
    const uint32_t mw = ix.mw;
    const size_t piece = std::max<size_t>(64, (((size_t)64 << 20) / (mw * 4)) & ~(size_t)63); // rows, whole blocks of 64
    std::vector<uint32_t> buf;
    for (size_t r0 = 0; codes && r0 < ix.n; r0 += piece)
    {
        const size_t cnt = std::min(piece, ix.n - r0), words = round_up(cnt, 64) * mw;
        buf.resize(words);
        MSVS_HIP(hipMemcpyAsync(buf.data(), ix.codes.p + r0 * mw, words * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        for (size_t r = 0; r < cnt; r++)
            for (size_t s = 0; s < ix.m; s++)
                codes[(r0 + r) * ix.m + s] = (uint8_t)(buf[pq_code_word(r, (uint32_t)(s >> 2), mw)] >> (8 * (s & 3)));
    }
    if (ids && ix.n)
    {
        std::vector<uint32_t> l32(ix.n);
        MSVS_HIP(hipMemcpyAsync(l32.data(), ix.labels.p, ix.n * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < ix.n; i++)
            ids[i] = (int64_t)l32[i];
    }
}

extern "C" int msvs_pq_index_export(const msvs_pq_index_t * ix, float * centroids, float * codebooks, int64_t * list_off, uint8_t * codes,
                                    int64_t * ids)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index has no codebook yet (train / set_codebook)");
        if (centroids)
            memcpy(centroids, ix->h_cent.data(), ix->h_cent.size() * 4);
        if (codebooks)
            memcpy(codebooks, ix->h_cb.data(), ix->h_cb.size() * 4);
        if (!list_off && !codes && !ids)
            return;
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index is not built: it has no lists to export");
        if (list_off)
            memcpy(list_off, ix->h_list_off.data(), (ix->nlist + 1) * 8);
        pq_fetch(*ix, codes, ids, thread_stream());
    });
}

namespace
{
struct PqHeader // 64 bytes, little endian
{
    char magic[8]; // "MSVSPQ01"
    uint32_t version; // 1
    int32_t metric;
    uint64_t dim, m, nlist, n;
    uint64_t reserved;
    uint64_t check; // FNV-1a of the bytes before it
};
struct PqIdHeader // 24 bytes
{
    char magic[8]; // "MSVSPQID"
    uint64_t n;
    uint64_t check;
};
}

extern "C" int msvs_pq_index_serialize_io(const msvs_pq_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index is not built");
        std::vector<uint8_t> codes(ix->n * ix->m);
        std::vector<int64_t> ids(ix->n);
        pq_fetch(*ix, codes.data(), ids.data(), thread_stream());
        {
            IoStream f(io, "pq_data", 1);
            PqHeader h{};
            memcpy(h.magic, "MSVSPQ01", 8);
            h.version = 1;
            h.metric = ix->metric;
            h.dim = ix->dim;
            h.m = ix->m;
            h.nlist = ix->nlist;
            h.n = ix->n;
            h.check = fnv1a(&h, offsetof(PqHeader, check));
            f.write(&h, sizeof(h));
            f.write(ix->h_cent.data(), ix->h_cent.size() * 4);
            f.write(ix->h_cb.data(), ix->h_cb.size() * 4);
            f.write(ix->h_list_off.data(), (ix->nlist + 1) * 8);
            if (!codes.empty())
                f.write(codes.data(), codes.size());
            f.finish();
        }
        {
            IoStream f(io, "pq_ids", 1);
            PqIdHeader h{};
            memcpy(h.magic, "MSVSPQID", 8);
            h.n = ix->n;
            h.check = fnv1a(&h, offsetof(PqIdHeader, check));
            f.write(&h, sizeof(h));
            if (ix->n)
                f.write(ids.data(), ix->n * 8);
            f.finish();
        }
    });
}

extern "C" int msvs_pq_index_load_io(const msvs_io_t * io, msvs_pq_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        *out = nullptr;
        std::unique_ptr<msvs_pq_index> ix(new msvs_pq_index);
        MSVS_HIP(hipGetDevice(&ix->device));
        hipStream_t stream = thread_stream();
        std::vector<float> cent, cb;
        std::vector<uint8_t> codes;
        std::vector<int64_t> ids;
        {
            IoStream f(io, "pq_data", 0);
            PqHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSPQ01", 8) != 0 || h.version != 1 || h.check != fnv1a(&h, offsetof(PqHeader, check))
                || (h.metric != MSVS_METRIC_L2 && h.metric != MSVS_METRIC_IP && h.metric != MSVS_METRIC_COSINE) || h.dim > 8192 || h.m > 128
                || !pq_fits((size_t)h.dim, (size_t)h.m) || h.nlist == 0 || h.nlist > 0x7fffffffull || h.n > 0xfffffff0ull || h.reserved != 0)
                fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index header");
            pq_set_geometry(*ix, h.metric, (size_t)h.dim, (size_t)h.m);
            ix->nlist = (size_t)h.nlist;
            ix->n = (size_t)h.n;
            read_grow(f, cent, ix->nlist * ix->dim);
            read_grow(f, cb, PQ_KSUB * ix->dim);
            read_grow(f, ix->h_list_off, ix->nlist + 1);
            const std::string bad = list_offsets_error(ix->h_list_off, ix->n, "msvs IVFPQ index");
            if (!bad.empty())
                fail(MSVS_ERR_IO, "%s", bad.c_str());
            ix->max_list_len = longest_list(ix->h_list_off);
            read_grow(f, codes, ix->n * ix->m);
            expect_end(f);
            for (float v : cb)
                if (!std::isfinite(v))
                    fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index: a codebook entry is not finite");
        }
        {
            IoStream f(io, "pq_ids", 0);
            PqIdHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSPQID", 8) != 0 || h.check != fnv1a(&h, offsetof(PqIdHeader, check)) || h.n != ix->n)
                fail(MSVS_ERR_IO, "corrupt msvs IVFPQ id list header");
            read_grow(f, ids, ix->n);
            expect_end(f);
            for (int64_t id : ids)
                if (id < 0 || id >= (int64_t)PQ_LABEL_END)
                    fail(MSVS_ERR_IO, "corrupt msvs IVFPQ id list: label %lld outside [0, 2^32 - 1)", (long long)id);
        }
        // the stored form: code words in transposed blocks of 64 rows, labels as u32
        ix->centroids.alloc(ix->nlist * ix->ld);
        upload_rows(ix->centroids.p, cent.data(), ix->nlist, (uint32_t)ix->dim, ix->ld, MSVS_MEM_HOST, stream);
        MSVS_HIP(hipStreamSynchronize(stream));
        pq_set_codebooks(*ix, cb.data(), stream);
        const uint32_t mw = ix->mw;
        const size_t code_words = std::max<size_t>(round_up(ix->n, 64), 64) * mw;
        ix->codes.alloc(code_words);
        ix->labels.alloc(std::max<size_t>(ix->n, 1));
        ix->list_off.alloc(ix->nlist + 1);
        MSVS_HIP(hipMemsetAsync(ix->codes.p, 0, code_words * 4, stream));
        const size_t piece = std::max<size_t>(64, (((size_t)64 << 20) / (mw * 4)) & ~(size_t)63);
        std::vector<uint32_t> buf;
        for (size_t r0 = 0; r0 < ix->n; r0 += piece)
        {
            const size_t cnt = std::min(piece, ix->n - r0), words = round_up(cnt, 64) * mw;
            buf.assign(words, 0);
            for (size_t r = 0; r < cnt; r++)
                for (size_t s = 0; s < ix->m; s++)
                    buf[pq_code_word(r, (uint32_t)(s >> 2), mw)] |= (uint32_t)codes[(r0 + r) * ix->m + s] << (8 * (s & 3));
            MSVS_HIP(hipMemcpyAsync(ix->codes.p + r0 * mw, buf.data(), words * 4, hipMemcpyHostToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        std::vector<uint32_t> l32(ix->n);
        for (size_t i = 0; i < ix->n; i++)
            l32[i] = (uint32_t)ids[i];
        if (ix->n)
            MSVS_HIP(hipMemcpyAsync(ix->labels.p, l32.data(), ix->n * 4, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipMemcpyAsync(ix->list_off.p, ix->h_list_off.data(), (ix->nlist + 1) * 8, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        MSVS_HIP(hipDeviceSynchronize());
        ix->staged = ix->n;
        ix->ready = true;
        *out = ix.release();
    });
}
