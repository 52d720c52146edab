// sq_index.hip -- the IVFSQ index (include/msvs.h: msvs_sq_index_*): coarse centroids + ONE per-dimension 8-bit quantiser of the
// residuals; codes, lists and labels are all the index keeps.  Semantics and layout: sq_ivf_kernels.hpp, DESIGN.md 4.11.
// Reused as they are: the k-means trainer (a temporary IVFFLAT index), the assignment kernel, flat_search_device for the coarse
// step, launch_ivf_plan, launch_ivf_merge, Scratch, normalize_device_rows, upload_rows.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "index_internal.hpp"
#include "io_stream.hpp"
#include "ivf_build_kernels.hpp"
#include "list_layout.hpp"
#include "sq_ivf_kernels.hpp"

using namespace msvs;

namespace
{
constexpr size_t SQ_ADD_ROWS = 65536;  // rows of a chunk on the device as f32 at a time (encode, range)
constexpr uint32_t SQ_LABEL_END = 0xffffffffu; // labels are < this

/// ldc: bytes of a stored row = floats of a padded query / centroid row
inline uint32_t sq_ld(size_t dim) { return (uint32_t)round_up(dim, (size_t)16); }
/// the smallest tile with the largest k must fit the scan's LDS budget
inline bool sq_fits(size_t dim) { return dim >= 1 && dim <= 8192 && sq_lds_bytes(2, sq_ld(dim) / 4, MSVS_MAX_K) <= SCAN_LDS_BUDGET; }

inline float sq_ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
}

struct msvs_sq_index
{
    int metric = MSVS_METRIC_L2;
    size_t dim = 0;
    uint32_t ld = 0; // round_up(dim, 16): floats per centroid / query row, bytes per stored row
    int device = 0;
    std::string params; // create's, handed to the temporary IVFFLAT index that runs the k-means
    // codebook
    size_t nlist = 0;
    DevBuf<float> centroids;      // nlist x ld
    std::vector<float> h_cent;    // nlist x dim
    std::vector<float> h_vmin, h_vmax; // dim
    DevBuf<float> d_vmin, d_step; // ld each, zero padded
    bool trained = false;
    // staging (between add and build): codes, list and label only
    struct Chunk
    {
        DevBuf<uint8_t> codes; // n x ld, stored order
        std::vector<int32_t> list;
        std::vector<int64_t> ids;
        size_t n = 0;
    };
    std::vector<Chunk> chunks;
    size_t staged = 0;
    // final storage
    DevBuf<uint8_t> codes;    // n x ld, list-major
    DevBuf<uint32_t> labels;  // n
    DevBuf<int64_t> list_off; // nlist + 1
    std::vector<int64_t> h_list_off;
    size_t n = 0, max_list_len = 0;
    bool ready = false;
};

/// centroids (nlist x ld on the device already) + quantiser bounds -> the index's codebook
static void sq_set_quantiser(msvs_sq_index & ix, const float * vmin, const float * vmax, hipStream_t stream)
{
    const size_t d = ix.dim;
    ix.h_vmin.assign(vmin, vmin + d);
    ix.h_vmax.assign(vmax, vmax + d);
    std::vector<float> pm(ix.ld, 0.f), ps(ix.ld, 0.f);
    for (size_t j = 0; j < d; j++)
    {
        const float range = vmax[j] - vmin[j];
        pm[j] = vmin[j];
        ps[j] = range / 255.0f;
    }
    ix.d_vmin.alloc(ix.ld);
    ix.d_step.alloc(ix.ld);
    MSVS_HIP(hipMemcpyAsync(ix.d_vmin.p, pm.data(), ix.ld * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipMemcpyAsync(ix.d_step.p, ps.data(), ix.ld * 4, hipMemcpyHostToDevice, stream));
    ix.h_cent.resize(ix.nlist * d);
    MSVS_HIP(hipMemcpy2DAsync(ix.h_cent.data(), d * 4, ix.centroids.p, (size_t)ix.ld * 4, d * 4, ix.nlist, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream)); // pm, ps are about to go
    ix.trained = true;
}

/// nearest centroid of n device rows (stride ld): by L2 for L2 indexes, by inner product for IP and cosine (as msvs_index_add)
static void sq_assign(const msvs_sq_index & ix, const float * d_x, size_t n, int32_t * d_assign, float * d_cnorm, hipStream_t stream)
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
static void sq_stage_rows(const msvs_sq_index & ix, const float * x, size_t m, int mem, float * d_x, int32_t * d_assign, float * d_cnorm,
                          hipStream_t stream)
{
    upload_rows(d_x, x, m, (uint32_t)ix.dim, ix.ld, mem, stream);
    if (ix.metric == MSVS_METRIC_COSINE)
        normalize_device_rows(d_x, m, (uint32_t)ix.dim, ix.ld, stream);
    sq_assign(ix, d_x, m, d_assign, d_cnorm, stream);
}

static void sq_check_codebook_time(const msvs_sq_index * ix)
{
    if (ix->staged || ix->ready)
        fail(MSVS_ERR_INVALID_ARGUMENT, "the codebook must be set before data is added");
}

extern "C" int msvs_sq_index_create(int metric, size_t dim, const char * params, msvs_sq_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        *out = nullptr;
        if (metric != MSVS_METRIC_L2 && metric != MSVS_METRIC_IP && metric != MSVS_METRIC_COSINE)
            fail(MSVS_ERR_NOT_IMPLEMENTED, "metric %d is not implemented for the IVFSQ index", metric);
        if (!sq_fits(dim))
            fail(MSVS_ERR_INVALID_ARGUMENT, "dimension %zu out of range for the IVFSQ index (the list scan's LDS stage holds up to 2240)", dim);
        auto p = parse_params(params);
        if (param_int(p, "ncentroids", 1024) < 1)
            fail(MSVS_ERR_INVALID_ARGUMENT, "bad ncentroids");
        std::unique_ptr<msvs_sq_index> ix(new msvs_sq_index);
        ix->metric = metric;
        ix->dim = dim;
        ix->ld = sq_ld(dim);
        ix->params = params ? params : "";
        MSVS_HIP(hipGetDevice(&ix->device));
        *out = ix.release();
    });
}

extern "C" void msvs_sq_index_free(msvs_sq_index_t * ix) { delete ix; }

extern "C" int msvs_sq_index_set_codebook(msvs_sq_index_t * ix, const float * centroids, size_t nlist, const float * vmin, const float * vmax,
                                          int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || !centroids || !vmin || !vmax || nlist == 0 || nlist > 0x7fffffffull)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / codebook");
        sq_check_codebook_time(ix);
        hipStream_t stream = thread_stream();
        std::vector<float> lo(ix->dim), hi(ix->dim);
        if (mem == MSVS_MEM_DEVICE)
        {
            MSVS_HIP(hipMemcpyAsync(lo.data(), vmin, ix->dim * 4, hipMemcpyDeviceToHost, stream));
            MSVS_HIP(hipMemcpyAsync(hi.data(), vmax, ix->dim * 4, hipMemcpyDeviceToHost, stream));
        }
        else
        {
            memcpy(lo.data(), vmin, ix->dim * 4);
            memcpy(hi.data(), vmax, ix->dim * 4);
        }
        ix->trained = false;
        ix->nlist = nlist;
        ix->centroids.alloc(nlist * ix->ld);
        upload_rows(ix->centroids.p, centroids, nlist, (uint32_t)ix->dim, ix->ld, mem, stream);
        MSVS_HIP(hipStreamSynchronize(stream));
        for (size_t j = 0; j < ix->dim; j++)
            if (!std::isfinite(lo[j]) || !std::isfinite(hi[j]) || hi[j] < lo[j])
            {
                ix->nlist = 0;
                ix->centroids.release();
                fail(MSVS_ERR_INVALID_ARGUMENT, "quantiser bounds of dimension %zu are not finite or vmax < vmin", j);
            }
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
    });
}

extern "C" int msvs_sq_index_train(msvs_sq_index_t * ix, const float * x, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || (n && !x))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / data");
        sq_check_codebook_time(ix);
        if (n == 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "no training data");
        hipStream_t stream = thread_stream();
        ix->trained = false;
        {
            // the coarse centroids: the IVFFLAT trainer as it is, through a temporary index of the same metric and parameters
            msvs_index_t * tmp = nullptr;
            int rc = msvs_index_create(MSVS_INDEX_IVFFLAT, ix->metric, ix->dim, ix->params.c_str(), &tmp);
            if (rc == MSVS_OK)
                rc = msvs_index_train(tmp, x, n, mem);
            if (rc != MSVS_OK)
            {
                const std::string why = msvs_last_error();
                msvs_index_free(tmp);
                fail(rc, "%s", why.c_str());
            }
            std::unique_ptr<msvs_index_t, void (*)(msvs_index_t *)> hold(tmp, msvs_index_free);
            ix->nlist = tmp->nlist;
            ix->centroids.alloc(ix->nlist * ix->ld);
            MSVS_HIP(hipMemsetAsync(ix->centroids.p, 0, ix->nlist * ix->ld * 4, stream));
            MSVS_HIP(hipMemcpy2DAsync(ix->centroids.p, (size_t)ix->ld * 4, tmp->centroids.p, (size_t)tmp->ld * 4, ix->dim * 4, ix->nlist,
                                      hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        // the quantiser: exact minimum / maximum of the residuals of every training row against its assigned centroid
        const size_t step_rows = std::min(n, SQ_ADD_ROWS);
        DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist);
        DevBuf<int32_t> d_assign(step_rows);
        DevBuf<uint32_t> d_range(2 * ix->dim);
        MSVS_HIP(hipMemsetAsync(d_range.p, 0xff, ix->dim * 4, stream));
        MSVS_HIP(hipMemsetAsync(d_range.p + ix->dim, 0, ix->dim * 4, stream));
        for (size_t r0 = 0; r0 < n; r0 += step_rows)
        {
            const size_t m = std::min(step_rows, n - r0);
            sq_stage_rows(*ix, x + r0 * ix->dim, m, mem, d_x.p, d_assign.p, d_cnorm.p, stream);
            const uint32_t rpb = 64;
            hipLaunchKernelGGL(sq_range_kernel, dim3((unsigned)ceil_div(m, (size_t)rpb)), dim3(BLOCK), 0, stream, d_x.p, d_assign.p,
                               ix->centroids.p, m, (uint32_t)ix->dim, ix->ld, rpb, d_range.p, d_range.p + ix->dim);
            MSVS_HIP(hipGetLastError());
        }
        std::vector<uint32_t> range(2 * ix->dim);
        MSVS_HIP(hipMemcpyAsync(range.data(), d_range.p, range.size() * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        std::vector<float> lo(ix->dim), hi(ix->dim);
        for (size_t j = 0; j < ix->dim; j++)
        {
            const bool seen = range[j] <= range[ix->dim + j]; // (a column of NaNs: the empty range 0 .. 0)
            lo[j] = seen ? sq_ord2f(range[j]) : 0.f;
            hi[j] = seen ? sq_ord2f(range[ix->dim + j]) : 0.f;
        }
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
    });
}

extern "C" int msvs_sq_index_add(msvs_sq_index_t * ix, const float * x, const int64_t * ids, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix || (n && !x))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / data");
        if (ix->ready)
            fail(MSVS_ERR_INVALID_ARGUMENT, "index already built");
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index has no codebook yet (train / set_codebook)");
        if (n == 0)
            return;
        if (ix->staged + n > 0xfffffff0ull)
            fail(MSVS_ERR_ID_RANGE, "more rows than the u32 row range");
        hipStream_t stream = thread_stream();
        msvs_sq_index::Chunk ch;
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
            if (ch.ids[i] < 0 || ch.ids[i] >= (int64_t)SQ_LABEL_END)
                fail(MSVS_ERR_ID_RANGE, "id %lld is outside the label range [0, 2^32 - 1)", (long long)ch.ids[i]);
        ch.codes.alloc(n * ix->ld);
        ch.list.resize(n);
        const size_t step_rows = std::min(n, SQ_ADD_ROWS);
        DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist);
        DevBuf<int32_t> d_assign(step_rows);
        for (size_t r0 = 0; r0 < n; r0 += step_rows)
        {
            const size_t m = std::min(step_rows, n - r0);
            sq_stage_rows(*ix, x + r0 * ix->dim, m, mem, d_x.p, d_assign.p, d_cnorm.p, stream);
            hipLaunchKernelGGL(sq_encode_kernel, dim3((unsigned)ceil_div(m * ix->ld, (size_t)BLOCK)), dim3(BLOCK), 0, stream, d_x.p, d_assign.p,
                               ix->centroids.p, ix->d_vmin.p, ix->d_step.p, m, (uint32_t)ix->dim, ix->ld, ix->ld, ch.codes.p + r0 * ix->ld);
            MSVS_HIP(hipGetLastError());
            MSVS_HIP(hipMemcpyAsync(ch.list.data() + r0, d_assign.p, m * 4, hipMemcpyDeviceToHost, stream));
            MSVS_HIP(hipStreamSynchronize(stream)); // d_x is reused by the next step
        }
        for (size_t i = 0; i < n; i++)
            if (ch.list[i] < 0 || (size_t)ch.list[i] >= ix->nlist)
                fail(MSVS_ERR_DEVICE, "internal: row %zu was assigned to list %d of %zu", i, ch.list[i], ix->nlist);
        ix->staged += n;
        ix->chunks.push_back(std::move(ch));
    });
}

extern "C" int msvs_sq_index_build(msvs_sq_index_t * ix)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (ix->ready)
            return;
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index has no codebook yet (train / set_codebook)");
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
        ix->codes.alloc(std::max<size_t>(n, 1) * ix->ld);
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
            const size_t m = ix->chunks[c].n;
            DevBuf<uint32_t> d_pos(m);
            MSVS_HIP(hipMemcpyAsync(d_pos.p, pos.data() + first, m * 4, hipMemcpyHostToDevice, stream));
            const uint32_t ld16 = ix->ld / 16;
            hipLaunchKernelGGL(sq_scatter_rows_kernel, dim3((unsigned)ceil_div(m * ld16, (size_t)256)), dim3(256), 0, stream,
                               reinterpret_cast<const uint4 *>(ix->chunks[c].codes.p), reinterpret_cast<uint4 *>(ix->codes.p), d_pos.p, m, ld16);
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

extern "C" int msvs_sq_index_ready(const msvs_sq_index_t * ix) { return ix && ix->ready ? 1 : 0; }
extern "C" size_t msvs_sq_index_num_data(const msvs_sq_index_t * ix) { return ix ? (ix->ready ? ix->n : ix->staged) : 0; }
extern "C" size_t msvs_sq_index_num_lists(const msvs_sq_index_t * ix) { return ix ? ix->nlist : 0; }
extern "C" size_t msvs_sq_index_memory_usage(const msvs_sq_index_t * ix)
{
    if (!ix)
        return 0;
    size_t b = ix->codes.bytes() + ix->labels.bytes() + ix->list_off.bytes() + ix->centroids.bytes() + ix->d_vmin.bytes() + ix->d_step.bytes();
    for (const auto & ch : ix->chunks)
        b += ch.codes.bytes();
    return b;
}

// ------------------------------------------------------------------------------------------- search

template <int METRIC, int T>
static void sq_dispatch_r(uint32_t grid, const SqIvfParams & a, hipStream_t stream)
{
    const size_t lds = sq_lds_bytes(T, a.ld4, a.k);
    switch (r_for_k(a.k))
    {
        case 1:
            hipLaunchKernelGGL((sq_ivf_scan_kernel<METRIC, T, 1>), dim3(grid), dim3(BLOCK), lds, stream, a);
            break;
        case 2:
            hipLaunchKernelGGL((sq_ivf_scan_kernel<METRIC, T, 2>), dim3(grid), dim3(BLOCK), lds, stream, a);
            break;
        default:
            hipLaunchKernelGGL((sq_ivf_scan_kernel<METRIC, T, 4>), dim3(grid), dim3(BLOCK), lds, stream, a);
            break;
    }
}

template <int METRIC>
static void sq_dispatch_t(uint32_t T, uint32_t grid, const SqIvfParams & a, hipStream_t stream)
{
    switch (T)
    {
        case 2:
            sq_dispatch_r<METRIC, 2>(grid, a, stream);
            break;
        case 4:
            sq_dispatch_r<METRIC, 4>(grid, a, stream);
            break;
        default:
            sq_dispatch_r<METRIC, 8>(grid, a, stream);
            break;
    }
}

/// Everything on the device, enqueued on `stream`: queries padded (and normalised for cosine) into scratch, the canonical coarse
/// quantiser over the centroids, the plan, the list scan over the codes, the per-query merge.
static void sq_search_device(const msvs_sq_index & ix, const float * d_queries, size_t nq, size_t k, size_t nprobe, const uint64_t * d_alive,
                             size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    check_k(k);
    if (!ix.ready)
        fail(MSVS_ERR_NOT_READY, "the IVFSQ index is not built");
    if (nprobe < 1)
        fail(MSVS_ERR_INVALID_ARGUMENT, "nprobe must be >= 1");
    if (nq == 0 || k == 0)
        return;
    if (!d_queries || !d_ids || !d_dis)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    const size_t nlist = ix.nlist, P = std::min(nprobe, nlist);
    if (P > MSVS_MAX_K)
        fail(MSVS_ERR_UNSUPPORTED_K, "min(nprobe, nlist) = %zu exceeds the coarse quantiser's top-k limit %d", P, MSVS_MAX_K);
    const uint32_t ld = ix.ld, ld4 = ld / 4;
    const int m = scan_metric(ix.metric);
    // row segments of whole 16-row steps; per query of a round: its padded row, its probes and pairs
    const SegmentPlan sp = plan_segments(ix.max_list_len, options().sq_ivf_rpb, 16, P, k, (size_t)ld * 4 + P * 8 + 64, nq);
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
        flat_search_device(scr, m, ix.centroids.p, nullptr, nlist, ld, dq, nqc, (uint32_t)P, nullptr, 0, co, stream);
        // 2. (query, list) pairs grouped by list -> (list, query tile, row segment) items
        const size_t n_pairs = nqc * P;
        uint32_t T = n_pairs >= 16 * nlist ? 8 : (n_pairs >= 2 * nlist ? 4 : 2);
        while (T > 2 && sq_lds_bytes(T, ld4, (uint32_t)k) > SCAN_LDS_BUDGET)
            T /= 2;
        plan.run(probes, ix.list_off.p, n_pairs, rpb, T, stream);
        // 3. the list scan over the codes
        SqIvfParams a{};
        a.codes = reinterpret_cast<const uint4 *>(ix.codes.p);
        a.labels = ix.labels.p;
        a.alive = d_alive;
        a.nbits = (uint32_t)std::min<size_t>(nbits, 0xffffffffu);
        a.Q = reinterpret_cast<const float4 *>(dq);
        a.cent = reinterpret_cast<const float4 *>(ix.centroids.p);
        a.vmin = reinterpret_cast<const float4 *>(ix.d_vmin.p);
        a.step = reinterpret_cast<const float4 *>(ix.d_step.p);
        a.partial = partial;
        a.ld4 = ld4;
        a.k = (uint32_t)k;
        a.nprobe = (uint32_t)P;
        a.nlist = (uint32_t)nlist;
        a.rows_per_block = rpb;
        a.seg_max = (uint32_t)seg_max;
        a.list_off = ix.list_off.p;
        a.pair_off = plan.pair_off;
        a.work_off = plan.work_off;
        a.pairs = plan.pairs;
        {
            ProfileScope prof("sq_ivf_scan", stream);
            const uint32_t grid = (uint32_t)std::min<size_t>(2048, n_pairs * seg_max);
            if (m == M_IP)
                sq_dispatch_t<M_IP>(T, grid, a, stream);
            else
                sq_dispatch_t<M_L2>(T, grid, a, stream);
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
        launch_ivf_merge(m, im, (uint32_t)nqc, stream);
    }
}

extern "C" int msvs_sq_index_search_device(const msvs_sq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                           const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] {
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        sq_search_device(*ix, d_queries, nq, k, nprobe, d_alive_bits, nbits, d_ids, d_dis, as_stream(hip_stream));
    });
}

extern "C" int msvs_sq_index_search(const msvs_sq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                    const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        const size_t nprobe = parse_nprobe(params);
        check_k(k);
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index is not built");
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
        sq_search_device(*ix, dq, nq, k, nprobe, d_alive, nbits, d_ids, d_dis, stream);
        MSVS_HIP(hipMemcpyAsync(ids, d_ids, nq * k * 8, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipMemcpyAsync(dis, d_dis, nq * k * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
    });
}

// ------------------------------------------------------------------------------------------- export and files

/// the built index's codes in NATURAL column order (n x dim) and its labels, on the host
static void sq_fetch(const msvs_sq_index & ix, uint8_t * codes, int64_t * ids, hipStream_t stream)
{
    const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / ix.ld);
    std::vector<uint8_t> buf;
    for (size_t r0 = 0; codes && r0 < ix.n; r0 += piece)
    {
        const size_t m = std::min(piece, ix.n - r0);
        buf.resize(m * ix.ld);
        MSVS_HIP(hipMemcpyAsync(buf.data(), ix.codes.p + r0 * ix.ld, m * ix.ld, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        for (size_t r = 0; r < m; r++)
            for (size_t j = 0; j < ix.dim; j++)
                codes[(r0 + r) * ix.dim + j] = buf[r * ix.ld + sq_stored_pos((uint32_t)j, ix.ld)];
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

extern "C" int msvs_sq_index_export(const msvs_sq_index_t * ix, float * centroids, float * vmin, float * vmax, int64_t * list_off, uint8_t * codes,
                                    int64_t * ids)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (!ix->trained)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index has no codebook yet (train / set_codebook)");
        if (centroids)
            memcpy(centroids, ix->h_cent.data(), ix->h_cent.size() * 4);
        if (vmin)
            memcpy(vmin, ix->h_vmin.data(), ix->dim * 4);
        if (vmax)
            memcpy(vmax, ix->h_vmax.data(), ix->dim * 4);
        if (!list_off && !codes && !ids)
            return;
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index is not built: it has no lists to export");
        if (list_off)
            memcpy(list_off, ix->h_list_off.data(), (ix->nlist + 1) * 8);
        sq_fetch(*ix, codes, ids, thread_stream());
    });
}

namespace
{
struct SqHeader // 56 bytes, little endian
{
    char magic[8]; // "MSVSSQ01"
    uint32_t version; // 1
    int32_t metric;
    uint64_t dim, nlist, n;
    uint64_t reserved;
    uint64_t check; // FNV-1a of the bytes before it
};
struct SqIdHeader // 24 bytes
{
    char magic[8]; // "MSVSSQID"
    uint64_t n;
    uint64_t check;
};
}

extern "C" int msvs_sq_index_serialize_io(const msvs_sq_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (!ix->ready)
            fail(MSVS_ERR_NOT_READY, "the IVFSQ index is not built");
        std::vector<uint8_t> codes(ix->n * ix->dim);
        std::vector<int64_t> ids(ix->n);
        sq_fetch(*ix, codes.data(), ids.data(), thread_stream());
        {
            IoStream f(io, "sq_data", 1);
            SqHeader h{};
            memcpy(h.magic, "MSVSSQ01", 8);
            h.version = 1;
            h.metric = ix->metric;
            h.dim = ix->dim;
            h.nlist = ix->nlist;
            h.n = ix->n;
            h.check = fnv1a(&h, offsetof(SqHeader, check));
            f.write(&h, sizeof(h));
            f.write(ix->h_cent.data(), ix->h_cent.size() * 4);
            f.write(ix->h_vmin.data(), ix->dim * 4);
            f.write(ix->h_vmax.data(), ix->dim * 4);
            f.write(ix->h_list_off.data(), (ix->nlist + 1) * 8);
            if (!codes.empty())
                f.write(codes.data(), codes.size());
            f.finish();
        }
        {
            IoStream f(io, "sq_ids", 1);
            SqIdHeader h{};
            memcpy(h.magic, "MSVSSQID", 8);
            h.n = ix->n;
            h.check = fnv1a(&h, offsetof(SqIdHeader, check));
            f.write(&h, sizeof(h));
            if (ix->n)
                f.write(ids.data(), ix->n * 8);
            f.finish();
        }
    });
}

extern "C" int msvs_sq_index_load_io(const msvs_io_t * io, msvs_sq_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        *out = nullptr;
        std::unique_ptr<msvs_sq_index> ix(new msvs_sq_index);
        MSVS_HIP(hipGetDevice(&ix->device));
        hipStream_t stream = thread_stream();
        std::vector<float> cent, lo, hi;
        std::vector<uint8_t> codes;
        std::vector<int64_t> ids;
        {
            IoStream f(io, "sq_data", 0);
            SqHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSSQ01", 8) != 0 || h.version != 1 || h.check != fnv1a(&h, offsetof(SqHeader, check))
                || (h.metric != MSVS_METRIC_L2 && h.metric != MSVS_METRIC_IP && h.metric != MSVS_METRIC_COSINE) || h.dim > 8192 || !sq_fits(h.dim)
                || h.nlist == 0 || h.nlist > 0x7fffffffull || h.n > 0xfffffff0ull)
                fail(MSVS_ERR_IO, "corrupt msvs IVFSQ index header");
            ix->metric = h.metric;
            ix->dim = (size_t)h.dim;
            ix->ld = sq_ld(ix->dim);
            ix->nlist = (size_t)h.nlist;
            ix->n = (size_t)h.n;
            read_grow(f, cent, ix->nlist * ix->dim);
            read_grow(f, lo, ix->dim);
            read_grow(f, hi, ix->dim);
            read_grow(f, ix->h_list_off, ix->nlist + 1);
            const std::string bad = list_offsets_error(ix->h_list_off, ix->n, "msvs IVFSQ index");
            if (!bad.empty())
                fail(MSVS_ERR_IO, "%s", bad.c_str());
            ix->max_list_len = longest_list(ix->h_list_off);
            read_grow(f, codes, ix->n * ix->dim);
            expect_end(f);
        }
        {
            IoStream f(io, "sq_ids", 0);
            SqIdHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSSQID", 8) != 0 || h.check != fnv1a(&h, offsetof(SqIdHeader, check)) || h.n != ix->n)
                fail(MSVS_ERR_IO, "corrupt msvs IVFSQ id list header");
            read_grow(f, ids, ix->n);
            expect_end(f);
            for (int64_t id : ids)
                if (id < 0 || id >= (int64_t)SQ_LABEL_END)
                    fail(MSVS_ERR_IO, "corrupt msvs IVFSQ id list: label %lld outside [0, 2^32 - 1)", (long long)id);
        }
        // the stored form: columns permuted per row, labels as u32
        ix->centroids.alloc(ix->nlist * ix->ld);
        upload_rows(ix->centroids.p, cent.data(), ix->nlist, (uint32_t)ix->dim, ix->ld, MSVS_MEM_HOST, stream);
        MSVS_HIP(hipStreamSynchronize(stream));
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
        ix->codes.alloc(std::max<size_t>(ix->n, 1) * ix->ld);
        ix->labels.alloc(std::max<size_t>(ix->n, 1));
        ix->list_off.alloc(ix->nlist + 1);
        const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / ix->ld);
        std::vector<uint8_t> buf;
        for (size_t r0 = 0; r0 < ix->n; r0 += piece)
        {
            const size_t m = std::min(piece, ix->n - r0);
            buf.assign(m * ix->ld, 0);
            for (size_t r = 0; r < m; r++)
                for (size_t j = 0; j < ix->dim; j++)
                    buf[r * ix->ld + sq_stored_pos((uint32_t)j, ix->ld)] = codes[(r0 + r) * ix->dim + j];
            MSVS_HIP(hipMemcpyAsync(ix->codes.p + r0 * ix->ld, buf.data(), m * ix->ld, hipMemcpyHostToDevice, stream));
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
