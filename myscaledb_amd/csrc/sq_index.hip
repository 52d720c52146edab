// sq_index.hip -- the IVFSQ index (include/msvs.h: msvs_sq_index_*): coarse centroids + ONE per-dimension 8-bit quantiser of the
// residuals (bit_size=4: 4-bit; bit_size=16: binary16 residuals, no quantiser in the arithmetic); codes, lists and labels are all
// the index keeps.  Semantics and layout: sq_ivf_kernels.hpp, sq_layout.hpp, DESIGN.md 4.11.
// Here: the geometry, the quantiser (bounds, range pass), the scan's shapes and dispatch, the data file and the stored order of a
// row.  Everything the index has in common with IVFPQ -- staging, add, build, the search skeleton, labels, the id file -- is
// coded_ivf.hpp, which also lists what is reused as it is.
#include <cmath>

#include "coded_ivf.hpp"
#include "sq_ivf_kernels.hpp"

using namespace msvs;

namespace
{
constexpr const char * SQ = "IVFSQ";

/// floats of a padded query / centroid row (= bytes of a stored row at 8 bits)
inline uint32_t sq_ld(size_t dim) { return (uint32_t)round_up(dim, (size_t)16); }
/// the smallest tile with the largest k must fit the scan's LDS budget (the 8-bit image: no width has a larger one)
inline bool sq_fits(size_t dim) { return dim >= 1 && dim <= 8192 && sq_lds_bytes(2, sq_ld(dim) / 4, MSVS_MAX_K) <= SCAN_LDS_BUDGET; }

inline float sq_ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
}

struct msvs_sq_index : CodedIvf // ld = round_up(dim, 16), row_bytes = 16 sq_row_words(bits, ld); codes: max(n, 1) rows, not zeroed
{
    uint32_t bits = 8;                 // 4, 8 or 16
    std::vector<float> h_vmin, h_vmax; // dim
    DevBuf<float> d_vmin, d_step;      // ld each, zero padded (bits 16: none, the range enters no arithmetic)
};

static void sq_set_geometry(msvs_sq_index & ix, int metric, size_t dim, uint32_t bits)
{
    ix.metric = metric;
    ix.dim = dim;
    ix.bits = bits;
    ix.ld = sq_ld(dim);
    ix.row_bytes = 16 * sq_row_words(bits, ix.ld);
}

/// bytes of a code in export's buffer (one code a byte at 4 and 8 bits, a little-endian uint16 at 16)
inline size_t sq_export_size(uint32_t bits) { return bits == 16 ? 2 : 1; }
/// bytes of a row in the data file: two codes a byte at 4 bits
inline size_t sq_file_row(uint32_t bits, size_t dim) { return bits == 4 ? (dim + 1) / 2 : dim * sq_export_size(bits); }

/// code of natural column j out of / into a stored row (sq_layout.hpp)
inline uint16_t sq_get(const uint8_t * row, uint32_t j, uint32_t ld, uint32_t bits)
{
    if (bits == 8)
        return row[sq_stored_pos(j, ld)];
    if (bits == 4)
    {
        const uint32_t p = sq4_stored_pos(j, ld);
        return (row[p >> 1] >> (4 * (p & 1))) & 15;
    }
    uint16_t h;
    memcpy(&h, row + 2 * (size_t)sq16_stored_pos(j, ld), 2);
    return h;
}

inline void sq_put(uint8_t * row, uint32_t j, uint32_t ld, uint32_t bits, uint16_t code) // (row: zeroed)
{
    if (bits == 8)
        row[sq_stored_pos(j, ld)] = (uint8_t)code;
    else if (bits == 4)
    {
        const uint32_t p = sq4_stored_pos(j, ld);
        row[p >> 1] |= (uint8_t)(code << (4 * (p & 1)));
    }
    else
        memcpy(row + 2 * (size_t)sq16_stored_pos(j, ld), &code, 2);
}

/// the first dimension whose bounds sq_set_quantiser cannot turn into a finite step (vmin, vmax or fl(vmax - vmin) is not finite), or
/// dim if there is none.  With an infinite step every code of the column is 0 and decodes to vmin + 0 * inf = NaN: the index would
/// build and never return a row.  At 16 bits the range enters no arithmetic and any range passes.
static size_t sq_unusable_dimension(uint32_t bits, const float * vmin, const float * vmax, size_t dim)
{
    for (size_t j = 0; bits != 16 && j < dim; j++)
        if (!std::isfinite(vmin[j]) || !std::isfinite(vmax[j]) || !std::isfinite(vmax[j] - vmin[j]))
            return j;
    return dim;
}

static void sq_drop_codebook(msvs_sq_index & ix)
{
    ix.trained = false;
    ix.nlist = 0;
    ix.centroids.release();
}

/// centroids (nlist x ld on the device already) + quantiser bounds (sq_unusable_dimension: none) -> the index's codebook
static void sq_set_quantiser(msvs_sq_index & ix, const float * vmin, const float * vmax, hipStream_t stream)
{
    const size_t d = ix.dim;
    ix.h_vmin.assign(vmin, vmin + d);
    ix.h_vmax.assign(vmax, vmax + d);
    if (ix.bits == 16)
    {
        finish_codebook(ix, stream);
        return;
    }
    std::vector<float> pm(ix.ld, 0.f), ps(ix.ld, 0.f);
    const float top = ix.bits == 4 ? 15.0f : 255.0f;
    for (size_t j = 0; j < d; j++)
    {
        const float range = vmax[j] - vmin[j];
        pm[j] = vmin[j];
        ps[j] = range / top;
    }
    ix.d_vmin.alloc(ix.ld);
    ix.d_step.alloc(ix.ld);
    MSVS_HIP(hipMemcpyAsync(ix.d_vmin.p, pm.data(), ix.ld * 4, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipMemcpyAsync(ix.d_step.p, ps.data(), ix.ld * 4, hipMemcpyHostToDevice, stream));
    finish_codebook(ix, stream); // (synchronises: pm, ps are about to go)
}

extern "C" int msvs_sq_index_create(int metric, size_t dim, const char * params, msvs_sq_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        check_metric(metric, SQ);
        if (!sq_fits(dim))
            fail(MSVS_ERR_INVALID_ARGUMENT, "dimension %zu out of range for the IVFSQ index (the list scan's LDS stage holds up to 2240)", dim);
        const auto p = parse_params(params);
        check_ncentroids(p);
        const long bits = param_int(p, "bit_size", 8);
        if (bits != 4 && bits != 8 && bits != 16)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the IVFSQ index has 4, 8 or 16 bits per dimension (bit_size %ld)", bits);
        std::unique_ptr<msvs_sq_index> ix(new msvs_sq_index);
        sq_set_geometry(*ix, metric, dim, (uint32_t)bits);
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
        check_codebook_time(*ix);
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
        upload_centroids(*ix, centroids, nlist, mem, stream);
        size_t bad = sq_unusable_dimension(ix->bits, lo.data(), hi.data(), ix->dim);
        for (size_t j = 0; j < bad; j++)
            if (!std::isfinite(lo[j]) || !std::isfinite(hi[j]) || hi[j] < lo[j])
                bad = j;
        if (bad < ix->dim)
        {
            sq_drop_codebook(*ix);
            fail(MSVS_ERR_INVALID_ARGUMENT, "quantiser bounds of dimension %zu are not finite, vmax < vmin or vmax - vmin overflows", bad);
        }
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
    });
}

extern "C" int msvs_sq_index_train(msvs_sq_index_t * ix, const float * x, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_rows(ix, x, n);
        check_codebook_time(*ix);
        if (n == 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "no training data");
        hipStream_t stream = thread_stream();
        ix->trained = false;
        train_centroids(*ix, x, n, mem, stream);
        // the quantiser: exact minimum / maximum of the residuals of every training row against its assigned centroid
        const size_t step_rows = std::min(n, CODED_ADD_ROWS);
        DevBuf<float> d_x(step_rows * ix->ld), d_cnorm(ix->nlist);
        DevBuf<int32_t> d_assign(step_rows);
        DevBuf<uint32_t> d_range(2 * ix->dim);
        MSVS_HIP(hipMemsetAsync(d_range.p, 0xff, ix->dim * 4, stream));
        MSVS_HIP(hipMemsetAsync(d_range.p + ix->dim, 0, ix->dim * 4, stream));
        for (size_t r0 = 0; r0 < n; r0 += step_rows)
        {
            const size_t m = std::min(step_rows, n - r0);
            stage_rows(*ix, x + r0 * ix->dim, m, mem, d_x.p, d_assign.p, d_cnorm.p, stream);
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
        const size_t bad = sq_unusable_dimension(ix->bits, lo.data(), hi.data(), ix->dim);
        if (bad < ix->dim)
        {
            sq_drop_codebook(*ix);
            fail(MSVS_ERR_INVALID_ARGUMENT,
                 "the training residuals of dimension %zu span %g .. %g: no finite quantiser step (an infinite or overflowing training row?)", bad,
                 (double)lo[bad], (double)hi[bad]);
        }
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
    });
}

extern "C" int msvs_sq_index_add(msvs_sq_index_t * ix, const float * x, const int64_t * ids, size_t n, int mem)
{
    return guarded([&] {
        add_rows(ix, x, ids, n, mem, SQ, false, [&](const float * d_x, const int32_t * d_assign, size_t m, uint8_t * dst, hipStream_t stream) {
            const uint32_t ldc = ix->bits == 4 ? ix->row_bytes : ix->ld; // elements of a row, one thread each
            with_int<8, 4, 16>((int)ix->bits, [&](auto b) {
                hipLaunchKernelGGL(sq_encode_kernel<decltype(b)::value>, dim3((unsigned)ceil_div(m * ldc, (size_t)BLOCK)), dim3(BLOCK), 0, stream,
                                   d_x, d_assign, ix->centroids.p, ix->d_vmin.p, ix->d_step.p, m, (uint32_t)ix->dim, ix->ld, ldc, dst);
            });
        });
    });
}

extern "C" int msvs_sq_index_build(msvs_sq_index_t * ix)
{
    return guarded([&] {
        build_lists(ix, SQ, 1, false, [&](const uint8_t * src, uint8_t * dst, const uint32_t * d_pos, size_t m, hipStream_t stream) {
            const uint32_t ld16 = ix->row_bytes / 16;
            hipLaunchKernelGGL(sq_scatter_rows_kernel, dim3((unsigned)ceil_div(m * ld16, (size_t)256)), dim3(256), 0, stream,
                               reinterpret_cast<const uint4 *>(src), reinterpret_cast<uint4 *>(dst), d_pos, m, ld16);
        });
    });
}

extern "C" int msvs_sq_index_ready(const msvs_sq_index_t * ix) { return ix && ix->ready ? 1 : 0; }
extern "C" size_t msvs_sq_index_num_data(const msvs_sq_index_t * ix) { return ix ? (ix->ready ? ix->n : ix->staged) : 0; }
extern "C" size_t msvs_sq_index_num_lists(const msvs_sq_index_t * ix) { return ix ? ix->nlist : 0; }
extern "C" size_t msvs_sq_index_bit_size(const msvs_sq_index_t * ix) { return ix ? ix->bits : 0; }
extern "C" size_t msvs_sq_index_memory_usage(const msvs_sq_index_t * ix)
{
    return ix ? coded_bytes(*ix) + ix->d_vmin.bytes() + ix->d_step.bytes() : 0;
}

// ------------------------------------------------------------------------------------------- search

/// tiles of 2, 4 or 8 queries (no T = 1).  A later rank round (a.after) takes the AFTER form, which exists with four top-k
/// registers per lane only: such a round follows one of MSVS_MAX_K ranks, and its own k is the search's remainder
template <int BITS>
static void launch_sq_ivf_scan(int metric, uint32_t T, uint32_t grid, const SqIvfParams & a, hipStream_t stream)
{
    with_int<M_IP, M_L2>(metric, [&](auto m) {
        with_int<2, 4, 8>(T, [&](auto t) {
            constexpr int METRIC = decltype(m)::value, TQ = decltype(t)::value;
            const size_t lds = sq_lds_bytes(TQ, a.ld4, a.k, BITS);
            if (a.after)
                hipLaunchKernelGGL((sq_ivf_scan_kernel<BITS, METRIC, TQ, 4, 1>), dim3(grid), dim3(BLOCK), lds, stream, a);
            else
                with_int<1, 2, 4>(r_for_k(a.k), [&](auto r) {
                    constexpr int R = decltype(r)::value;
                    hipLaunchKernelGGL((sq_ivf_scan_kernel<BITS, METRIC, TQ, R>), dim3(grid), dim3(BLOCK), lds, stream, a);
                });
        });
    });
}

/// search_device of coded_ivf.hpp with this index's shapes: row segments of whole 16-row steps, tiles of 2, 4 or 8 queries
static void sq_search_device(const msvs_sq_index & ix, const float * d_queries, size_t nq, size_t k, size_t k_max, size_t nprobe,
                             const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    const uint32_t ld4 = ix.ld / 4;
    search_device(
        ix, SQ, "sq_ivf_scan", d_queries, nq, k, k_max, nprobe, d_alive, nbits, d_ids, d_dis, stream, 16, options().sq_ivf_rpb,
        [&](size_t n_pairs, size_t k_) {
            uint32_t T = n_pairs >= 16 * ix.nlist ? 8 : (n_pairs >= 2 * ix.nlist ? 4 : 2);
            while (T > 2 && sq_lds_bytes(T, ld4, (uint32_t)k_, ix.bits) > SCAN_LDS_BUDGET)
                T /= 2;
            return T;
        },
        [&](uint32_t T, uint32_t grid, const ScanRound & r) {
            SqIvfParams a{};
            fill_scan_params(a, ix, r);
            a.codes = reinterpret_cast<const uint4 *>(ix.codes.p);
            a.Q = reinterpret_cast<const float4 *>(r.dq);
            a.cent = reinterpret_cast<const float4 *>(ix.centroids.p);
            a.vmin = reinterpret_cast<const float4 *>(ix.d_vmin.p);
            a.step = reinterpret_cast<const float4 *>(ix.d_step.p);
            a.ld4 = ld4;
            with_int<8, 4, 16>((int)ix.bits, [&](auto b) { launch_sq_ivf_scan<decltype(b)::value>(r.metric, T, grid, a, stream); });
        });
}

// The C entries come in two forms that differ in their limits alone: the one-round form (k, kc <= MSVS_MAX_K) and the rounds form
// (k <= MSVS_MAX_K_ROUNDS; kc <= MSVS_REFINE_MAX_CAND).

static int sq_search_device_entry(const msvs_sq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t k_max, size_t nprobe,
                                  const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] {
        check_index(ix);
        sq_search_device(*ix, d_queries, nq, k, k_max, nprobe, d_alive_bits, nbits, d_ids, d_dis, as_stream(hip_stream));
    });
}

static int sq_search_entry(const msvs_sq_index_t * ix, const float * queries, size_t nq, size_t k, size_t k_max, const char * params,
                           const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        search_host(ix, SQ, queries, nq, k, k_max, params, alive_bits, nbits, ids, dis,
                    [&](const float * dq, size_t nprobe, const uint64_t * d_alive, int64_t * d_ids, float * d_dis, hipStream_t stream) {
                        sq_search_device(*ix, dq, nq, k, k_max, nprobe, d_alive, nbits, d_ids, d_dis, stream);
                    });
    });
}

static int sq_search_refine_device_entry(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * d_queries, size_t nq, size_t k,
                                         size_t kc, size_t kc_max, size_t nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                         float * d_dis, void * hip_stream)
{
    return guarded([&] {
        check_index(ix);
        hipStream_t stream = as_stream(hip_stream);
        search_refine_device(*ix, SQ, rows, d_queries, nq, k, kc, kc_max, d_ids, d_dis, stream, [&](int64_t * c_ids, float * c_dis) {
            sq_search_device(*ix, d_queries, nq, kc, kc_max, nprobe, d_alive_bits, nbits, c_ids, c_dis, stream);
        });
    });
}

static int sq_search_refine_entry(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq, size_t k, size_t kc,
                                  size_t kc_max, const char * params, const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        search_host(ix, SQ, queries, nq, k, MSVS_MAX_K, params, alive_bits, nbits, ids, dis,
                    [&](const float * dq, size_t nprobe, const uint64_t * d_alive, int64_t * d_ids, float * d_dis, hipStream_t stream) {
                        search_refine_device(*ix, SQ, rows, dq, nq, k, kc, kc_max, d_ids, d_dis, stream, [&](int64_t * c_ids, float * c_dis) {
                            sq_search_device(*ix, dq, nq, kc, kc_max, nprobe, d_alive, nbits, c_ids, c_dis, stream);
                        });
                    });
    });
}

extern "C" int msvs_sq_index_search_device(const msvs_sq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                           const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return sq_search_device_entry(ix, d_queries, nq, k, MSVS_MAX_K, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_sq_index_search_rounds_device(const msvs_sq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                                  const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                  void * hip_stream)
{
    return sq_search_device_entry(ix, d_queries, nq, k, MSVS_MAX_K_ROUNDS, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_sq_index_search(const msvs_sq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                    const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return sq_search_entry(ix, queries, nq, k, MSVS_MAX_K, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_sq_index_search_rounds(const msvs_sq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                           const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return sq_search_entry(ix, queries, nq, k, MSVS_MAX_K_ROUNDS, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_sq_index_search_refine_device(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * d_queries, size_t nq,
                                                  size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits, size_t nbits,
                                                  int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return sq_search_refine_device_entry(ix, rows, d_queries, nq, k, kc, MSVS_MAX_K, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_sq_index_search_refine_rounds_device(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * d_queries,
                                                         size_t nq, size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits,
                                                         size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return sq_search_refine_device_entry(ix, rows, d_queries, nq, k, kc, MSVS_REFINE_MAX_CAND, nprobe, d_alive_bits, nbits, d_ids, d_dis,
                                         hip_stream);
}

extern "C" int msvs_sq_index_search_refine(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq, size_t k,
                                           size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits, int64_t * ids,
                                           float * dis)
{
    return sq_search_refine_entry(ix, rows, queries, nq, k, kc, MSVS_MAX_K, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_sq_index_search_refine_rounds(const msvs_sq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq,
                                                  size_t k, size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits,
                                                  int64_t * ids, float * dis)
{
    return sq_search_refine_entry(ix, rows, queries, nq, k, kc, MSVS_REFINE_MAX_CAND, params, alive_bits, nbits, ids, dis);
}

// ------------------------------------------------------------------------------------------- export and files

/// the built index's codes in NATURAL column order (n x dim; export's form: a byte a code, a little-endian uint16 at 16 bits) and
/// its labels, on the host
static void sq_fetch(const msvs_sq_index & ix, uint8_t * codes, int64_t * ids, hipStream_t stream)
{
    const size_t rb = ix.row_bytes, es = sq_export_size(ix.bits);
    const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / rb);
    std::vector<uint8_t> buf;
    for (size_t r0 = 0; codes && r0 < ix.n; r0 += piece)
    {
        const size_t m = std::min(piece, ix.n - r0);
        buf.resize(m * rb);
        MSVS_HIP(hipMemcpyAsync(buf.data(), ix.codes.p + r0 * rb, m * rb, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        for (size_t r = 0; r < m; r++)
            for (size_t j = 0; j < ix.dim; j++)
            {
                const uint16_t c = sq_get(&buf[r * rb], (uint32_t)j, ix.ld, ix.bits);
                memcpy(codes + ((r0 + r) * ix.dim + j) * es, &c, es); // (little endian: the low byte is the code at 4 and 8 bits)
            }
    }
    fetch_labels(ix, ids, stream);
}

extern "C" int msvs_sq_index_export(const msvs_sq_index_t * ix, float * centroids, float * vmin, float * vmax, int64_t * list_off, uint8_t * codes,
                                    int64_t * ids)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        export_head(ix, SQ, centroids);
        if (vmin)
            memcpy(vmin, ix->h_vmin.data(), ix->dim * 4);
        if (vmax)
            memcpy(vmax, ix->h_vmax.data(), ix->dim * 4);
        if (export_lists(*ix, SQ, list_off, codes, ids))
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
    uint64_t reserved; // the code width: 0 for 8 bits (the files of before bit_size), 4 or 16
    uint64_t check; // FNV-1a of the bytes before it
};
}

extern "C" int msvs_sq_index_serialize_io(const msvs_sq_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_index(ix);
        check_built(*ix, SQ);
        std::vector<uint8_t> codes(ix->n * ix->dim * sq_export_size(ix->bits));
        std::vector<int64_t> ids(ix->n);
        sq_fetch(*ix, codes.data(), ids.data(), thread_stream());
        if (ix->bits == 4) // the file keeps two codes a byte in natural order: code j in the low (even j) or high nibble of byte j / 2
        {
            const size_t fr = sq_file_row(4, ix->dim);
            std::vector<uint8_t> packed(ix->n * fr, 0);
            for (size_t r = 0; r < ix->n; r++)
                for (size_t j = 0; j < ix->dim; j++)
                    packed[r * fr + j / 2] |= (uint8_t)(codes[r * ix->dim + j] << (4 * (j & 1)));
            codes.swap(packed);
        }
        {
            IoStream f(io, "sq_data", 1);
            SqHeader h{};
            memcpy(h.magic, "MSVSSQ01", 8);
            h.version = 1;
            h.metric = ix->metric;
            h.dim = ix->dim;
            h.nlist = ix->nlist;
            h.n = ix->n;
            h.reserved = ix->bits == 8 ? 0 : ix->bits;
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
        write_id_file(io, "sq_ids", "MSVSSQID", ids);
    });
}

extern "C" int msvs_sq_index_load_io(const msvs_io_t * io, msvs_sq_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        std::unique_ptr<msvs_sq_index> ix(new msvs_sq_index);
        MSVS_HIP(hipGetDevice(&ix->device));
        hipStream_t stream = thread_stream();
        std::vector<float> cent, lo, hi;
        std::vector<uint8_t> codes;
        {
            IoStream f(io, "sq_data", 0);
            SqHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSSQ01", 8) != 0 || h.version != 1 || h.check != fnv1a(&h, offsetof(SqHeader, check))
                || !header_ranges_ok(h.metric, h.dim, h.nlist, h.n) || !sq_fits(h.dim) || (h.reserved != 0 && h.reserved != 4 && h.reserved != 16))
                fail(MSVS_ERR_IO, "corrupt msvs IVFSQ index header");
            sq_set_geometry(*ix, h.metric, (size_t)h.dim, h.reserved ? (uint32_t)h.reserved : 8);
            ix->nlist = (size_t)h.nlist;
            ix->n = (size_t)h.n;
            read_grow(f, cent, ix->nlist * ix->dim);
            read_grow(f, lo, ix->dim);
            read_grow(f, hi, ix->dim);
            read_list_offsets(f, *ix, SQ);
            read_grow(f, codes, ix->n * sq_file_row(ix->bits, ix->dim));
            expect_end(f);
            const size_t bad = sq_unusable_dimension(ix->bits, lo.data(), hi.data(), ix->dim);
            if (bad < ix->dim)
                fail(MSVS_ERR_IO, "corrupt msvs IVFSQ index: the quantiser bounds of dimension %zu give no finite step", bad);
            if (ix->bits == 4 && (ix->dim & 1))
                for (size_t r = 0, fr = sq_file_row(4, ix->dim); r < ix->n; r++)
                    if (codes[r * fr + fr - 1] >> 4)
                        fail(MSVS_ERR_IO, "corrupt msvs IVFSQ index: a pad nibble of row %zu is not 0", r);
        }
        const std::vector<int64_t> ids = read_id_file(io, "sq_ids", "MSVSSQID", ix->n, SQ);
        // the stored form: columns permuted per row, labels as u32
        upload_centroids(*ix, cent.data(), ix->nlist, MSVS_MEM_HOST, stream);
        sq_set_quantiser(*ix, lo.data(), hi.data(), stream);
        alloc_lists(*ix, ix->n, 1, false, stream);
        const size_t rb = ix->row_bytes, fr = sq_file_row(ix->bits, ix->dim);
        const size_t piece = std::max<size_t>(1, ((size_t)64 << 20) / rb);
        std::vector<uint8_t> buf;
        for (size_t r0 = 0; r0 < ix->n; r0 += piece)
        {
            const size_t m = std::min(piece, ix->n - r0);
            buf.assign(m * rb, 0);
            for (size_t r = 0; r < m; r++)
            {
                const uint8_t * src = &codes[(r0 + r) * fr];
                for (size_t j = 0; j < ix->dim; j++)
                {
                    uint16_t c = 0;
                    if (ix->bits == 4)
                        c = (src[j / 2] >> (4 * (j & 1))) & 15;
                    else
                        memcpy(&c, src + j * sq_export_size(ix->bits), sq_export_size(ix->bits));
                    sq_put(&buf[r * rb], (uint32_t)j, ix->ld, ix->bits, c);
                }
            }
            MSVS_HIP(hipMemcpyAsync(ix->codes.p + r0 * rb, buf.data(), m * rb, hipMemcpyHostToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        finish_load(*ix, ids, stream);
        *out = ix.release();
    });
}
