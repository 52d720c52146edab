// refine.hip -- the row store (include/msvs.h: msvs_rows_*) and the second stage of a two-stage search (msvs_refine[_device]):
// the candidate labels a coded index returned, scored against the original f32 rows with the canonical arithmetic.  The kernel
// and its layout: refine_kernels.hpp; the composed entries of the coded indexes: coded_ivf.hpp (search_refine_device).
// DESIGN.md 4.13.
#include <algorithm>
#include <memory>

#include "coded_ivf.hpp"
#include "refine_kernels.hpp"

using namespace msvs;

static_assert(MSVS_REFINE_MAX_CAND <= 4 * BLOCK, "refine_kernel ranks at most four keys per thread");

// row i is label i; ld = round_up(dim, 4) floats a row, zero padded; the table is capacity x ld, in HBM or in mapped pinned host memory
struct msvs_rows
{
    size_t dim = 0, capacity = 0, n = 0;
    uint32_t ld = 0;
    int normalize = 0, placement = MSVS_ROWS_DEVICE, device = 0;
    DevBuf<float> dev;          // MSVS_ROWS_DEVICE
    float * host = nullptr;     // MSVS_ROWS_HOST_PINNED: the host address ...
    float * host_dev = nullptr; // ... and the address the kernel reads it at
    const float * table() const { return placement == MSVS_ROWS_DEVICE ? dev.p : host_dev; }
    ~msvs_rows()
    {
        if (host)
            (void)hipHostFree(host);
    }
};

namespace
{
constexpr size_t ROWS_STAGE_BYTES = (size_t)64 << 20; // device staging of an append to a pinned store, at most

/// rows [r0, r0 + cnt) of a pinned store that has to pass through the device (a device source, or rows to normalise)
void append_pinned_staged(msvs_rows & rs, const float * x, size_t n, int mem, hipStream_t stream)
{
    const size_t step = std::max<size_t>(1, std::min(n, ROWS_STAGE_BYTES / ((size_t)rs.ld * 4)));
    DevBuf<float> d_x(step * rs.ld);
    for (size_t r0 = 0; r0 < n; r0 += step)
    {
        const size_t cnt = std::min(step, n - r0);
        upload_rows(d_x.p, x + r0 * rs.dim, cnt, (uint32_t)rs.dim, rs.ld, mem, stream);
        if (rs.normalize)
            normalize_device_rows(d_x.p, cnt, (uint32_t)rs.dim, rs.ld, stream);
        MSVS_HIP(hipMemcpyAsync(rs.host + (rs.n + r0) * rs.ld, d_x.p, cnt * rs.ld * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream)); // d_x is reused by the next step
    }
}
}

extern "C" int msvs_rows_create(size_t dim, int normalize, int placement, size_t capacity_rows, msvs_rows_t ** out)
{
    return guarded([&] {
        clear_out(out);
        if (dim < 1 || dim > 8192)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the row store needs 1 <= dim <= 8192 (dim %zu)", dim);
        if (placement != MSVS_ROWS_DEVICE && placement != MSVS_ROWS_HOST_PINNED)
            fail(MSVS_ERR_INVALID_ARGUMENT, "placement %d is neither MSVS_ROWS_DEVICE nor MSVS_ROWS_HOST_PINNED", placement);
        if (capacity_rows > 0xffffffffull)
            fail(MSVS_ERR_ID_RANGE, "capacity %zu exceeds the label range: at most 2^32 - 1 rows", capacity_rows);
        std::unique_ptr<msvs_rows> rs(new msvs_rows);
        rs->dim = dim;
        rs->ld = padded_dim(dim);
        rs->capacity = capacity_rows;
        rs->normalize = normalize ? 1 : 0;
        rs->placement = placement;
        MSVS_HIP(hipGetDevice(&rs->device));
        const size_t bytes = capacity_rows * rs->ld * 4;
        if (placement == MSVS_ROWS_DEVICE)
            rs->dev.alloc(capacity_rows * rs->ld);
        else if (bytes)
        {
            void * p = nullptr;
            const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable);
            if (e != hipSuccess)
                fail(MSVS_ERR_OUT_OF_MEMORY, "hipHostMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
            rs->host = static_cast<float *>(p);
            void * d = nullptr;
            MSVS_HIP(hipHostGetDevicePointer(&d, p, 0));
            rs->host_dev = static_cast<float *>(d);
        }
        *out = rs.release();
    });
}

extern "C" void msvs_rows_free(msvs_rows_t * rows) { delete rows; }
extern "C" size_t msvs_rows_num(const msvs_rows_t * rows) { return rows ? rows->n : 0; }
extern "C" size_t msvs_rows_dim(const msvs_rows_t * rows) { return rows ? rows->dim : 0; }
extern "C" int msvs_rows_normalized(const msvs_rows_t * rows) { return rows ? rows->normalize : 0; }
extern "C" size_t msvs_rows_memory_usage(const msvs_rows_t * rows) { return rows ? rows->dev.bytes() : 0; }

extern "C" int msvs_rows_append(msvs_rows_t * rows, const float * x, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(rows ? rows->device : -1);
        if (!rows || (n && !x))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null row store / data");
        if (n > rows->capacity - rows->n)
            fail(MSVS_ERR_INVALID_ARGUMENT, "%zu rows more than the store's capacity (%zu of %zu rows are in)", n, rows->n, rows->capacity);
        if (n == 0)
            return;
        msvs_rows & rs = *rows;
        hipStream_t stream = thread_stream();
        if (rs.placement == MSVS_ROWS_DEVICE)
        {
            float * dst = rs.dev.p + rs.n * rs.ld;
            upload_rows(dst, x, n, (uint32_t)rs.dim, rs.ld, mem, stream);
            if (rs.normalize)
                normalize_device_rows(dst, n, (uint32_t)rs.dim, rs.ld, stream);
            MSVS_HIP(hipStreamSynchronize(stream));
            MSVS_HIP(hipDeviceSynchronize()); // refines run on other streams
        }
        else if (mem == MSVS_MEM_DEVICE || rs.normalize)
            append_pinned_staged(rs, x, n, mem, stream);
        else
            for (size_t r = 0; r < n; r++)
            {
                float * dst = rs.host + (rs.n + r) * rs.ld;
                memcpy(dst, x + r * rs.dim, rs.dim * 4);
                for (size_t c = rs.dim; c < rs.ld; c++)
                    dst[c] = 0.f;
            }
        rs.n += n;
    });
}

// ------------------------------------------------------------------------------------------- the second stage

/// what both entries check before anything is staged or enqueued; false: a no-op
static bool refine_checks(const msvs_rows * rows, int metric, const float * queries, size_t nq, const int64_t * cand, size_t kc, size_t k,
                          const int64_t * ids, const float * dis)
{
    if (!rows)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null row store");
    if (!metric_ok(metric))
        fail(MSVS_ERR_NOT_IMPLEMENTED, "metric %d is not implemented for the refine step", metric);
    if ((metric == MSVS_METRIC_COSINE) != (rows->normalize != 0))
        fail(MSVS_ERR_INVALID_ARGUMENT, "a cosine refine needs a row store created with normalize=1, L2 and IP one with normalize=0");
    check_k(k);
    if (kc > MSVS_REFINE_MAX_CAND)
        fail(MSVS_ERR_UNSUPPORTED_K, "kc = %zu exceeds the refine step's candidate limit %d", kc, MSVS_REFINE_MAX_CAND);
    if (nq > 0x7fffffffull)
        fail(MSVS_ERR_INVALID_ARGUMENT, "more than 2^31 - 1 queries in one refine (a block per query)");
    if (nq == 0 || k == 0)
        return false;
    if (!queries || !ids || !dis || (kc && !cand))
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    return true;
}

namespace msvs
{
void refine_device(const msvs_rows * rows, int metric, const float * d_queries, size_t nq, const int64_t * d_cand, size_t kc, size_t k,
                   int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    if (!refine_checks(rows, metric, d_queries, nq, d_cand, kc, k, d_ids, d_dis))
        return;
    const uint32_t ld = rows->ld;
    Scratch & scr = scratch_for(stream);
    scr.reserve(nq * ld * 4 + 2 * 256, stream);
    float * dq = scr.take<float>(nq * ld);
    upload_rows(dq, d_queries, nq, (uint32_t)rows->dim, ld, MSVS_MEM_DEVICE, stream);
    if (metric == MSVS_METRIC_COSINE)
        normalize_device_rows(dq, nq, (uint32_t)rows->dim, ld, stream);
    RefineParams a{};
    a.rows = reinterpret_cast<const float4 *>(rows->table());
    a.Q = reinterpret_cast<const float4 *>(dq);
    a.cand = d_cand;
    a.out_ids = d_ids;
    a.out_dis = d_dis;
    a.num = rows->n;
    a.ld4 = ld / 4;
    a.kc = (uint32_t)kc;
    a.k = (uint32_t)k;
    a.cosine = metric == MSVS_METRIC_COSINE;
    const size_t lds = refine_lds_bytes(a.ld4, a.kc); // <= 32 KiB of query + 8 KiB of keys
    ProfileScope prof("refine", stream);
    with_int<M_IP, M_L2>(scan_metric(metric), [&](auto m) {
        hipLaunchKernelGGL((refine_kernel<decltype(m)::value>), dim3((unsigned)nq), dim3(BLOCK), lds, stream, a); // a block per query
    });
    MSVS_HIP(hipGetLastError());
}
}

extern "C" int msvs_refine_device(const msvs_rows_t * rows, int metric, const float * d_queries, size_t nq, const int64_t * d_cand, size_t kc,
                                  size_t k, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] { refine_device(rows, metric, d_queries, nq, d_cand, kc, k, d_ids, d_dis, as_stream(hip_stream)); });
}

extern "C" int msvs_refine(const msvs_rows_t * rows, int metric, const float * queries, size_t nq, const int64_t * cand, size_t kc, size_t k,
                           int64_t * ids, float * dis)
{
    return guarded([&] {
        DeviceGuard on_device(rows ? rows->device : -1);
        hipStream_t stream = thread_stream();
        if (!refine_checks(rows, metric, queries, nq, cand, kc, k, ids, dis))
            return;
        const size_t dim = rows->dim;
        Scratch & stg = staging_for(stream);
        stg.reserve(nq * dim * 4 + nq * kc * 8 + nq * k * 12 + 5 * 256, stream);
        float * dq = stg.take<float>(nq * dim);
        int64_t * d_cand = stg.take<int64_t>(nq * kc);
        int64_t * d_ids = stg.take<int64_t>(nq * k);
        float * d_dis = stg.take<float>(nq * k);
        MSVS_HIP(hipMemcpyAsync(dq, queries, nq * dim * 4, hipMemcpyHostToDevice, stream));
        if (kc)
            MSVS_HIP(hipMemcpyAsync(d_cand, cand, nq * kc * 8, hipMemcpyHostToDevice, stream));
        refine_device(rows, metric, dq, nq, d_cand, kc, k, d_ids, d_dis, stream);
        MSVS_HIP(hipMemcpyAsync(ids, d_ids, nq * k * 8, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipMemcpyAsync(dis, d_dis, nq * k * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
    });
}
