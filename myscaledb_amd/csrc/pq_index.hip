// pq_index.hip -- the IVFPQ index (include/msvs.h: msvs_pq_index_*): coarse centroids + m sub-quantisers of 256 (bit_size 8) or 16
// (bit_size 4) entries over the residuals; codes, lists and labels are all the index keeps.  Semantics and layout: pq_ivf_kernels.hpp, DESIGN.md 4.12.
// Here: the geometry, the sub-codebooks (finiteness, residual sampling, training), the scan's shapes, LDS attribute and dispatch,
// the data file and the stored order of the code words, the form (query_tables) with its row terms and per-query tables.
// Everything the index has in common with IVFSQ -- staging, add, build, the search skeleton, labels, the id file -- is
// coded_ivf.hpp, which also lists what is reused as it is.
#include <cmath>
#include <mutex>

#include "coded_ivf.hpp"
#include "pq_ivf_kernels.hpp"

using namespace msvs;

namespace
{
constexpr const char * PQ = "IVFPQ";
constexpr size_t PQ_TRAIN_ROWS = 262144; // residuals the sub-codebooks are trained on at most

/// sub-quantisers an index of this bit size has at most: a stored row stays within 128 bytes
inline size_t pq_max_m(size_t bits) { return 1024 / bits; }

/// dim / m / bit size of an index that can exist: the smallest tile with the largest k must fit the scan's LDS
inline bool pq_fits(size_t dim, size_t m, size_t bits)
{
    if ((bits != 4 && bits != 8) || dim < 1 || dim > 8192 || m < 1 || m > pq_max_m(bits) || dim % m != 0)
        return false;
    return pq_lds_bytes(bits, 1, (uint32_t)m, padded_dim(dim), MSVS_MAX_K) <= PQ_LDS_BUDGET;
}
}

// ld = round_up(dim, 4); row_bytes = 4 * mw; codes: round_up(max(n, 1), 64) rows, zeroed, list-major, blocks of 64 rows transposed
// (pq_code_word); a staged chunk: n x mw words, row-major, zeroed
struct msvs_pq_index : CodedIvf
{
    size_t m = 0, dsub = 0;
    size_t bits = 8, ksub = 256; // bits of a code, entries of a sub-codebook (1 << bits)
    uint32_t mw = 0;         // 32-bit words of a stored row: ceil(m / 4), 4-bit: ceil(m / 8)
    std::vector<float> h_cb; // [m][ksub][dsub]
    DevBuf<float> cbT;       // the same in the order of pq_cb_index
    int form = 0;            // query_tables: 1 = tables that depend on the query alone (pq_ivf_kernels.hpp)
    DevBuf<float> row_w;     // form 1, L2: the row term of every list-major row (max(n, 1) floats), else empty
    bool keeps_row_terms() const { return form == 1 && metric == MSVS_METRIC_L2; }
    const uint32_t * code_words() const { return reinterpret_cast<const uint32_t *>(codes.p); }
};

/// the row terms of a built or loaded index that keeps them: allocated and computed from the stored codes (build and load_io both
/// end here, so the two cannot drift apart); synchronises
static void pq_compute_row_terms(msvs_pq_index & ix, hipStream_t stream)
{
    if (!ix.keeps_row_terms())
        return;
    ix.row_w.alloc(std::max<size_t>(ix.n, 1));
    MSVS_HIP(hipMemsetAsync(ix.row_w.p, 0, ix.row_w.bytes(), stream));
    if (ix.n)
        with_int<8, 4>((int)ix.bits, [&](auto b) {
            hipLaunchKernelGGL((pq_row_terms_kernel<decltype(b)::value>), dim3((unsigned)ceil_div(ix.n, (size_t)256)), dim3(256), 0, stream,
                               ix.code_words(), ix.list_off.p, ix.centroids.p, ix.cbT.p, ix.n, (uint32_t)ix.nlist, ix.ld, (uint32_t)ix.m,
                               (uint32_t)ix.dsub, ix.mw, ix.row_w.p);
        });
    MSVS_HIP(hipGetLastError());
    MSVS_HIP(hipStreamSynchronize(stream));
    MSVS_HIP(hipDeviceSynchronize()); // searches run on other streams
}

static void pq_set_geometry(msvs_pq_index & ix, int metric, size_t dim, size_t m, size_t bits)
{
    ix.bits = bits;
    ix.ksub = (size_t)1 << bits;
    ix.metric = metric;
    ix.dim = dim;
    ix.m = m;
    ix.dsub = dim / m;
    ix.ld = padded_dim(dim);
    ix.mw = (uint32_t)ceil_div(m, (size_t)(32 / bits));
    ix.row_bytes = ix.mw * 4;
}

/// centroids (nlist x ld on the device already) + sub-codebooks [m][ksub][dsub] on the host -> the index's codebook
static void pq_set_codebooks(msvs_pq_index & ix, const float * cb, hipStream_t stream)
{
    const size_t d = ix.dim, m = ix.m, dsub = ix.dsub, ksub = ix.ksub;
    for (size_t i = 0; i < ksub * d; i++)
        if (!std::isfinite(cb[i]))
            fail(MSVS_ERR_INVALID_ARGUMENT, "codebook entry %zu of sub-quantiser %zu is not finite", (i / dsub) % ksub, i / (ksub * dsub));
    ix.h_cb.assign(cb, cb + ksub * d);
    std::vector<float> t(ksub * d);
    with_int<8, 4>((int)ix.bits, [&](auto b) {
        for (uint32_t s = 0; s < m; s++)
            for (uint32_t j = 0; j < ksub; j++)
                for (uint32_t u = 0; u < dsub; u++)
                    t[pq_cb_index<decltype(b)::value>(s, u, j, (uint32_t)m, (uint32_t)dsub)] = cb[((size_t)s * ksub + j) * dsub + u];
    });
    ix.cbT.alloc(ksub * d);
    MSVS_HIP(hipMemcpyAsync(ix.cbT.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, stream));
    finish_codebook(ix, stream); // (synchronises: t is about to go)
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

/// pq_set_codebooks; a refused codebook leaves none
static void pq_set_codebooks_or_drop(msvs_pq_index & ix, const float * cb, hipStream_t stream)
{
    try
    {
        pq_set_codebooks(ix, cb, stream);
    }
    catch (...)
    {
        pq_drop_codebook(ix);
        throw;
    }
}

extern "C" int msvs_pq_index_create(int metric, size_t dim, const char * params, msvs_pq_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        check_metric(metric, PQ);
        auto p = parse_params(params);
        check_ncentroids(p);
        const long m = param_int(p, "m", 0), bits = param_int(p, "bit_size", 8);
        if (bits != 4 && bits != 8)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the IVFPQ index has 4 or 8 bits per sub-quantiser (bit_size %ld)", bits);
        const long form = param_int(p, "query_tables", 0);
        if (form != 0 && form != 1)
            fail(MSVS_ERR_INVALID_ARGUMENT, "query_tables is 0 or 1 (%ld)", form);
        if (m < 1 || !pq_fits(dim, (size_t)m, (size_t)bits))
            fail(MSVS_ERR_INVALID_ARGUMENT,
                 "the IVFPQ index needs 1 <= m <= 128 (256 at bit_size=4) dividing 1 <= dim <= 8192 and tables of m KiB (m / 16 KiB) + 8 * dim + "
                 "10 KiB within 160 KiB (dim %zu, m %ld, bit_size %ld)",
                 dim, m, bits);
        std::unique_ptr<msvs_pq_index> ix(new msvs_pq_index);
        pq_set_geometry(*ix, metric, dim, (size_t)m, (size_t)bits);
        ix->form = (int)form;
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
        check_codebook_time(*ix);
        hipStream_t stream = thread_stream();
        std::vector<float> cb(ix->ksub * ix->dim);
        if (mem == MSVS_MEM_DEVICE)
            MSVS_HIP(hipMemcpyAsync(cb.data(), codebooks, cb.size() * 4, hipMemcpyDeviceToHost, stream));
        else
            memcpy(cb.data(), codebooks, cb.size() * 4);
        pq_drop_codebook(*ix);
        upload_centroids(*ix, centroids, nlist, mem, stream);
        ix->nlist = nlist;
        pq_set_codebooks_or_drop(*ix, cb.data(), stream);
    });
}

extern "C" int msvs_pq_index_train(msvs_pq_index_t * ix, const float * x, size_t n, int mem)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_rows(ix, x, n);
        check_codebook_time(*ix);
        const size_t ksub = ix->ksub;
        if (n < ksub)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the IVFPQ index needs at least %zu training rows (%zu given)", ksub, n);
        hipStream_t stream = thread_stream();
        const size_t d = ix->dim, m = ix->m, dsub = ix->dsub;
        pq_drop_codebook(*ix);
        train_centroids(*ix, x, n, mem, stream);
        {
            // a NaN or infinite training row in the coarse trainer's sample ends in the mean of its list; the sub-codebooks trained on the
            // residuals could still come out finite (the residual sample is another one), so the coarse centroids are checked here
            std::vector<float> hc(ix->nlist * d);
            MSVS_HIP(hipMemcpy2D(hc.data(), d * 4, ix->centroids.p, (size_t)ix->ld * 4, d * 4, ix->nlist, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < hc.size(); i++)
                if (!std::isfinite(hc[i]))
                {
                    pq_drop_codebook(*ix);
                    fail(MSVS_ERR_INVALID_ARGUMENT, "coarse centroid %zu is not finite: a training row is NaN, infinite or overflows", i / d);
                }
        }
        // the residuals fl(x - c_l) of the evenly spaced training rows floor(i * n / cap), dense on the device
        const size_t cap = std::min(n, PQ_TRAIN_ROWS);
        DevBuf<float> d_res(cap * d);
        {
            const size_t step_rows = std::min(cap, CODED_ADD_ROWS);
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
                stage_rows(*ix, src, cnt, src_mem, d_x.p, d_assign.p, d_cnorm.p, stream);
                hipLaunchKernelGGL(pq_residual_kernel, dim3((unsigned)ceil_div(cnt * d, (size_t)256)), dim3(256), 0, stream, d_x.p, d_assign.p,
                                   ix->centroids.p, cnt, (uint32_t)d, ix->ld, d_res.p + i0 * d);
                MSVS_HIP(hipGetLastError());
                MSVS_HIP(hipStreamSynchronize(stream)); // d_x / h_pick are reused by the next step
            }
        }
        // every sub-codebook: the same trainer over the sub-space's columns, L2, ksub centroids, the caller's iterations and seed
        std::string sub_params;
        for (const auto & kv : parse_params(ix->params.c_str()))
            if (kv.first != "ncentroids" && kv.first != "m" && kv.first != "bit_size" && kv.first != "query_tables")
                sub_params += kv.first + "=" + kv.second + ",";
        sub_params += "ncentroids=" + std::to_string(ksub);
        DevBuf<float> d_sub(cap * dsub);
        std::vector<float> cb(ksub * d);
        for (size_t s = 0; s < m; s++)
        {
            MSVS_HIP(hipMemcpy2DAsync(d_sub.p, dsub * 4, d_res.p + s * dsub, d * 4, dsub * 4, cap, hipMemcpyDeviceToDevice, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
            const TmpIndex tmp = kmeans(MSVS_METRIC_L2, dsub, sub_params, d_sub.p, cap, MSVS_MEM_DEVICE);
            if (tmp->nlist != ksub)
                fail(MSVS_ERR_DEVICE, "internal: sub-quantiser %zu came out with %zu centroids", s, tmp->nlist);
            MSVS_HIP(hipMemcpy2D(cb.data() + s * ksub * dsub, dsub * 4, tmp->centroids.p, (size_t)tmp->ld * 4, dsub * 4, ksub,
                                 hipMemcpyDeviceToHost));
        }
        pq_set_codebooks_or_drop(*ix, cb.data(), stream);
    });
}

extern "C" int msvs_pq_index_add(msvs_pq_index_t * ix, const float * x, const int64_t * ids, size_t n, int mem)
{
    return guarded([&] {
        add_rows(ix, x, ids, n, mem, PQ, true, [&](const float * d_x, const int32_t * d_assign, size_t cnt, uint8_t * dst, hipStream_t stream) {
            if (ix->bits == 4)
            {
                hipLaunchKernelGGL(pq4_encode_kernel, dim3((unsigned)ceil_div(cnt, (size_t)16)), dim3(BLOCK), 0, stream, d_x, d_assign,
                                   ix->centroids.p, ix->cbT.p, cnt, ix->ld, (uint32_t)ix->m, (uint32_t)ix->dsub, ix->mw * 4, dst);
                return;
            }
            // the encoder stages a row and its centroid in LDS: more than 64 KiB of it (dim > 8184, beside its 64 static bytes) needs the
            // attribute raised once
            static std::once_flag once;
            std::call_once(once, [] {
                MSVS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&pq_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             2 * 8192 * 4));
            });
            const uint32_t rpb = 8;
            hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)ceil_div(cnt, (size_t)rpb)), dim3(BLOCK), 2 * ix->dim * 4, stream, d_x, d_assign,
                               ix->centroids.p, ix->cbT.p, cnt, (uint32_t)ix->dim, ix->ld, (uint32_t)ix->m, (uint32_t)ix->dsub, ix->mw * 4, rpb, dst);
        });
    });
}

extern "C" int msvs_pq_index_build(msvs_pq_index_t * ix)
{
    return guarded([&] {
        const bool was_ready = ix && ix->ready;
        build_lists(ix, PQ, 64, true, [&](const uint8_t * src, uint8_t * dst, const uint32_t * d_pos, size_t cnt, hipStream_t stream) {
            hipLaunchKernelGGL(pq_scatter_rows_kernel, dim3((unsigned)ceil_div(cnt * ix->mw, (size_t)256)), dim3(256), 0, stream,
                               reinterpret_cast<const uint32_t *>(src), reinterpret_cast<uint32_t *>(dst), d_pos, cnt, ix->mw);
        });
        if (!was_ready)
        {
            DeviceGuard on_device(ix->device);
            pq_compute_row_terms(*ix, thread_stream());
        }
    });
}

extern "C" int msvs_pq_index_ready(const msvs_pq_index_t * ix) { return ix && ix->ready ? 1 : 0; }
extern "C" size_t msvs_pq_index_num_data(const msvs_pq_index_t * ix) { return ix ? (ix->ready ? ix->n : ix->staged) : 0; }
extern "C" size_t msvs_pq_index_num_lists(const msvs_pq_index_t * ix) { return ix ? ix->nlist : 0; }
extern "C" size_t msvs_pq_index_memory_usage(const msvs_pq_index_t * ix)
{
    return ix ? coded_bytes(*ix) + ix->cbT.bytes() + ix->row_w.bytes() : 0;
}
extern "C" size_t msvs_pq_index_bit_size(const msvs_pq_index_t * ix) { return ix ? ix->bits : 0; }
extern "C" int msvs_pq_index_query_tables(const msvs_pq_index_t * ix) { return ix ? ix->form : 0; }

// ------------------------------------------------------------------------------------------- search

template <int BITS, int METRIC, int T, int R, int FORM, int AFTER = 0>
static void pq_launch(uint32_t grid, size_t lds, const PqIvfParams & a, hipStream_t stream)
{
    constexpr auto kernel = &pq_ivf_scan_kernel<BITS, METRIC, T, R, FORM, AFTER>;
    // more than 64 KiB of dynamic LDS needs the attribute raised once per kernel
    static std::once_flag once;
    std::call_once(once, [] {
        const void * fn = reinterpret_cast<const void *>(kernel);
        hipFuncAttributes fa{};
        MSVS_HIP(hipFuncGetAttributes(&fa, fn));
        if (fa.sharedSizeBytes != 0) // PQ_LDS_BUDGET: the dynamic image may be the whole LDS
            fail(MSVS_ERR_DEVICE, "the IVFPQ list scan has %zu bytes of static LDS: pq_fits no longer holds", (size_t)fa.sharedSizeBytes);
        MSVS_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQ_LDS_BUDGET));
    });
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), lds, stream, a);
}

/// tiles of 1, 2, 4 or 8 queries; 256- or 16-entry tables; built per (query, list) pair or copied from the query's (form).
/// A later rank round (a.after) takes the AFTER form, which exists with four top-k registers per lane only: such a round
/// follows one of MSVS_MAX_K ranks, and its own k is the search's remainder
static void launch_pq_ivf_scan(size_t bits, int form, int metric, uint32_t T, uint32_t grid, const PqIvfParams & a, hipStream_t stream)
{
    const size_t lds = pq_lds_bytes(bits, T, a.m, a.ld, a.k, form);
    with_int<1, 0>(form, [&](auto f) {
        with_int<8, 4>((int)bits, [&](auto b) {
            with_int<M_IP, M_L2>(metric, [&](auto m) {
                with_int<1, 2, 4, 8>(T, [&](auto t) {
                    if (a.after)
                        pq_launch<decltype(b)::value, decltype(m)::value, decltype(t)::value, 4, decltype(f)::value, 1>(grid, lds, a, stream);
                    else
                        with_int<1, 2, 4>(r_for_k(a.k), [&](auto r) {
                            pq_launch<decltype(b)::value, decltype(m)::value, decltype(t)::value, decltype(r)::value, decltype(f)::value>(
                                grid, lds, a, stream);
                        });
                });
            });
        });
    });
}

/// the tables of the nq padded queries of a round (form 1): P[query][s * ksub + j]
static void launch_pq_query_tables(const msvs_pq_index & ix, const float * dq, size_t nq, float * P, hipStream_t stream)
{
    constexpr int TQ = 8;
    ProfileScope prof("pq_query_tables", stream);
    with_int<8, 4>((int)ix.bits, [&](auto b) {
        constexpr int BITS = decltype(b)::value;
        const dim3 grid((unsigned)ceil_div(nq, (size_t)TQ), (unsigned)ceil_div(ix.m, (size_t)(BLOCK >> BITS)));
        hipLaunchKernelGGL((pq_query_table_kernel<BITS, TQ>), grid, dim3(BLOCK), 0, stream, dq, ix.cbT.p, (uint32_t)nq, ix.ld, (uint32_t)ix.m,
                           (uint32_t)ix.dsub, P);
    });
}

/// search_device of coded_ivf.hpp with this index's shapes: row segments of whole 256-row steps (a segment rebuilds its tile's
/// tables, or copies them in form 1); the tile by the pairs per list, 1 to 8 queries, halved until its tables fit.  Form 1 takes the
/// probes' distances from the coarse step and 4 * ksub * m bytes per query of the round for the query tables, from the same arena
static void pq_search_device(const msvs_pq_index & ix, const float * d_queries, size_t nq, size_t k, size_t k_max, size_t nprobe,
                             const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    if (ix.ready && ix.keeps_row_terms() && !ix.row_w.p)
        fail(MSVS_ERR_NOT_READY, "the IVFPQ index has no row terms: its build did not finish");
    RoundExtra extra;
    extra.bytes_per_q = ix.form ? ix.m * ix.ksub * 4 : 0;
    extra.probe_dis = ix.form != 0;
    search_device(
        ix, PQ, "pq_ivf_scan", d_queries, nq, k, k_max, nprobe, d_alive, nbits, d_ids, d_dis, stream, BLOCK, options().pq_ivf_rpb, extra,
        [&](size_t n_pairs, size_t k_) {
            const size_t nlist = ix.nlist;
            uint32_t T = n_pairs >= 16 * nlist ? 8 : (n_pairs >= 2 * nlist ? 4 : (n_pairs >= nlist ? 2 : 1));
            while (T > 1 && pq_lds_bytes(ix.bits, T, (uint32_t)ix.m, ix.ld, (uint32_t)k_, ix.form) > PQ_LDS_BUDGET)
                T /= 2;
            return T;
        },
        [&](const ScanRound & r) {
            if (ix.form)
                launch_pq_query_tables(ix, r.dq, r.nq, static_cast<float *>(r.extra), stream);
        },
        [&](uint32_t T, uint32_t grid, const ScanRound & r) {
            PqIvfParams a{};
            fill_scan_params(a, ix, r);
            a.codes = ix.code_words();
            a.Q = r.dq;
            a.cent = ix.centroids.p;
            a.cbT = ix.cbT.p;
            a.ld = ix.ld;
            a.dim = (uint32_t)ix.dim;
            a.m = (uint32_t)ix.m;
            a.dsub = (uint32_t)ix.dsub;
            a.mw = ix.mw;
            a.tables_only = options().pq_ivf_tables_only != 0;
            a.qtab = static_cast<const float *>(r.extra);
            a.pair_b = r.probe_dis;
            a.row_w = ix.row_w.p;
            launch_pq_ivf_scan(ix.bits, ix.form, r.metric, T, grid, a, stream);
        });
}

// The C entries come in two forms that differ in their limits alone: the one-round form (k, kc <= MSVS_MAX_K) and the rounds form
// (k <= MSVS_MAX_K_ROUNDS; kc <= MSVS_REFINE_MAX_CAND).

static int pq_search_device_entry(const msvs_pq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t k_max, size_t nprobe,
                                  const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] {
        check_index(ix);
        pq_search_device(*ix, d_queries, nq, k, k_max, nprobe, d_alive_bits, nbits, d_ids, d_dis, as_stream(hip_stream));
    });
}

static int pq_search_entry(const msvs_pq_index_t * ix, const float * queries, size_t nq, size_t k, size_t k_max, const char * params,
                           const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        search_host(ix, PQ, queries, nq, k, k_max, params, alive_bits, nbits, ids, dis,
                    [&](const float * dq, size_t nprobe, const uint64_t * d_alive, int64_t * d_ids, float * d_dis, hipStream_t stream) {
                        pq_search_device(*ix, dq, nq, k, k_max, nprobe, d_alive, nbits, d_ids, d_dis, stream);
                    });
    });
}

static int pq_search_refine_device_entry(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * d_queries, size_t nq, size_t k,
                                         size_t kc, size_t kc_max, size_t nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                         float * d_dis, void * hip_stream)
{
    return guarded([&] {
        check_index(ix);
        hipStream_t stream = as_stream(hip_stream);
        search_refine_device(*ix, PQ, rows, d_queries, nq, k, kc, kc_max, d_ids, d_dis, stream, [&](int64_t * c_ids, float * c_dis) {
            pq_search_device(*ix, d_queries, nq, kc, kc_max, nprobe, d_alive_bits, nbits, c_ids, c_dis, stream);
        });
    });
}

static int pq_search_refine_entry(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq, size_t k, size_t kc,
                                  size_t kc_max, const char * params, const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        search_host(ix, PQ, queries, nq, k, MSVS_MAX_K, params, alive_bits, nbits, ids, dis,
                    [&](const float * dq, size_t nprobe, const uint64_t * d_alive, int64_t * d_ids, float * d_dis, hipStream_t stream) {
                        search_refine_device(*ix, PQ, rows, dq, nq, k, kc, kc_max, d_ids, d_dis, stream, [&](int64_t * c_ids, float * c_dis) {
                            pq_search_device(*ix, dq, nq, kc, kc_max, nprobe, d_alive, nbits, c_ids, c_dis, stream);
                        });
                    });
    });
}

extern "C" int msvs_pq_index_search_device(const msvs_pq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                           const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return pq_search_device_entry(ix, d_queries, nq, k, MSVS_MAX_K, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_pq_index_search_rounds_device(const msvs_pq_index_t * ix, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                                  const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                  void * hip_stream)
{
    return pq_search_device_entry(ix, d_queries, nq, k, MSVS_MAX_K_ROUNDS, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_pq_index_search(const msvs_pq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                    const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return pq_search_entry(ix, queries, nq, k, MSVS_MAX_K, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_pq_index_search_rounds(const msvs_pq_index_t * ix, const float * queries, size_t nq, size_t k, const char * params,
                                           const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return pq_search_entry(ix, queries, nq, k, MSVS_MAX_K_ROUNDS, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_pq_index_search_refine_device(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * d_queries, size_t nq,
                                                  size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits, size_t nbits,
                                                  int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return pq_search_refine_device_entry(ix, rows, d_queries, nq, k, kc, MSVS_MAX_K, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_pq_index_search_refine_rounds_device(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * d_queries,
                                                         size_t nq, size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits,
                                                         size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return pq_search_refine_device_entry(ix, rows, d_queries, nq, k, kc, MSVS_REFINE_MAX_CAND, nprobe, d_alive_bits, nbits, d_ids, d_dis,
                                         hip_stream);
}

extern "C" int msvs_pq_index_search_refine(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq, size_t k,
                                           size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits, int64_t * ids,
                                           float * dis)
{
    return pq_search_refine_entry(ix, rows, queries, nq, k, kc, MSVS_MAX_K, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_pq_index_search_refine_rounds(const msvs_pq_index_t * ix, const msvs_rows_t * rows, const float * queries, size_t nq,
                                                  size_t k, size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits,
                                                  int64_t * ids, float * dis)
{
    return pq_search_refine_entry(ix, rows, queries, nq, k, kc, MSVS_REFINE_MAX_CAND, params, alive_bits, nbits, ids, dis);
}

// ------------------------------------------------------------------------------------------- export and files

/// bytes of a row's codes in the data file: they are the stored row's words, little endian, without the pad (8 bits: byte s is code
/// s; 4 bits: two codes a byte, even s in the low nibble)
static size_t pq_file_row_bytes(size_t m, size_t bits) { return ceil_div(m * bits, (size_t)8); }

/// The stored rows through the host, a piece of whole blocks of 64 rows at a time: fn(the piece's first row, its rows, its words
/// (pq_code_word from that row)), on the words that came down from the device (kind: device to host) or, zero before fn, go up after it.
template <typename F>
static void pq_each_piece(const msvs_pq_index & ix, hipMemcpyKind kind, hipStream_t stream, F && fn)
{
    const uint32_t mw = ix.mw;
    const size_t piece = std::max<size_t>(64, (((size_t)64 << 20) / (mw * 4)) & ~(size_t)63);
    std::vector<uint32_t> buf;
    for (size_t r0 = 0; r0 < ix.n; r0 += piece)
    {
        const size_t cnt = std::min(piece, ix.n - r0), words = round_up(cnt, 64) * mw;
        uint32_t * d_words = reinterpret_cast<uint32_t *>(ix.codes.p) + r0 * mw;
        buf.assign(words, 0);
        const bool down = kind == hipMemcpyDeviceToHost;
        if (!down)
            fn(r0, cnt, buf.data());
        MSVS_HIP(hipMemcpyAsync(down ? buf.data() : d_words, down ? d_words : buf.data(), words * 4, kind, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
        if (down)
            fn(r0, cnt, buf.data());
    }
}

/// code s of row r of a piece of stored rows (pq_code_word from the piece's first row)
static uint8_t pq_code_of(const uint32_t * words, size_t r, size_t s, uint32_t mw, size_t bits)
{
    const size_t cpw = 32 / bits, ksub = (size_t)1 << bits;
    return (uint8_t)((words[pq_code_word(r, (uint32_t)(s / cpw), mw)] >> (bits * (s % cpw))) & (ksub - 1));
}

/// the built index's codes in NATURAL order (n x m, one code a byte) and its labels, on the host
static void pq_fetch(const msvs_pq_index & ix, uint8_t * codes, int64_t * ids, hipStream_t stream)
{
    if (codes)
        pq_each_piece(ix, hipMemcpyDeviceToHost, stream, [&](size_t r0, size_t cnt, const uint32_t * words) {
            for (size_t r = 0; r < cnt; r++)
                for (size_t s = 0; s < ix.m; s++)
                    codes[(r0 + r) * ix.m + s] = pq_code_of(words, r, s, ix.mw, ix.bits);
        });
    fetch_labels(ix, ids, stream);
}

extern "C" int msvs_pq_index_export(const msvs_pq_index_t * ix, float * centroids, float * codebooks, int64_t * list_off, uint8_t * codes,
                                    int64_t * ids)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        export_head(ix, PQ, centroids);
        if (codebooks)
            memcpy(codebooks, ix->h_cb.data(), ix->h_cb.size() * 4);
        if (export_lists(*ix, PQ, list_off, codes, ids))
            pq_fetch(*ix, codes, ids, thread_stream());
    });
}

extern "C" int msvs_pq_index_export_row_terms(const msvs_pq_index_t * ix, float * w)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_index(ix);
        if (!ix->keeps_row_terms())
            fail(MSVS_ERR_INVALID_ARGUMENT, "the IVFPQ index keeps no row terms (query_tables=1 and L2 only)");
        check_built(*ix, PQ);
        if (!w)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
        if (!ix->n)
            return;
        if (!ix->row_w.p)
            fail(MSVS_ERR_NOT_READY, "the IVFPQ index has no row terms: its build did not finish");
        hipStream_t stream = thread_stream();
        MSVS_HIP(hipMemcpyAsync(w, ix->row_w.p, ix->n * 4, hipMemcpyDeviceToHost, stream));
        MSVS_HIP(hipStreamSynchronize(stream));
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
    uint64_t reserved; // 0: 8 bits per code, one code a byte; 4: 4 bits, two codes a byte (even s in the low nibble); + 0x100: query_tables=1
    uint64_t check; // FNV-1a of the bytes before it
};
}

extern "C" int msvs_pq_index_serialize_io(const msvs_pq_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        DeviceGuard on_device(ix ? ix->device : -1);
        check_index(ix);
        check_built(*ix, PQ);
        const size_t fb = pq_file_row_bytes(ix->m, ix->bits);
        std::vector<uint8_t> codes(ix->n * fb);
        std::vector<int64_t> ids(ix->n);
        pq_each_piece(*ix, hipMemcpyDeviceToHost, thread_stream(), [&](size_t r0, size_t cnt, const uint32_t * words) {
            for (size_t r = 0; r < cnt; r++)
                for (size_t i = 0; i < fb; i++)
                    codes[(r0 + r) * fb + i] = (uint8_t)(words[pq_code_word(r, (uint32_t)(i >> 2), ix->mw)] >> (8 * (i & 3)));
        });
        fetch_labels(*ix, ids.data(), thread_stream());
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
            h.reserved = (ix->bits == 4 ? 4 : 0) | (ix->form ? 0x100 : 0);
            h.check = fnv1a(&h, offsetof(PqHeader, check));
            f.write(&h, sizeof(h));
            f.write(ix->h_cent.data(), ix->h_cent.size() * 4);
            f.write(ix->h_cb.data(), ix->h_cb.size() * 4);
            f.write(ix->h_list_off.data(), (ix->nlist + 1) * 8);
            if (!codes.empty())
                f.write(codes.data(), codes.size());
            f.finish();
        }
        write_id_file(io, "pq_ids", "MSVSPQID", ids);
    });
}

extern "C" int msvs_pq_index_load_io(const msvs_io_t * io, msvs_pq_index_t ** out)
{
    return guarded([&] {
        clear_out(out);
        std::unique_ptr<msvs_pq_index> ix(new msvs_pq_index);
        MSVS_HIP(hipGetDevice(&ix->device));
        hipStream_t stream = thread_stream();
        std::vector<float> cent, cb;
        std::vector<uint8_t> codes;
        {
            IoStream f(io, "pq_data", 0);
            PqHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSPQ01", 8) != 0 || h.version != 1 || h.check != fnv1a(&h, offsetof(PqHeader, check))
                || !header_ranges_ok(h.metric, h.dim, h.nlist, h.n) || ((h.reserved & ~(uint64_t)0x100) != 0 && (h.reserved & ~(uint64_t)0x100) != 4))
                fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index header");
            const size_t bits = (h.reserved & 4) ? 4 : 8;
            ix->form = (h.reserved & 0x100) ? 1 : 0;
            if (h.m > pq_max_m(bits) || !pq_fits((size_t)h.dim, (size_t)h.m, bits))
                fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index header");
            pq_set_geometry(*ix, h.metric, (size_t)h.dim, (size_t)h.m, bits);
            ix->nlist = (size_t)h.nlist;
            ix->n = (size_t)h.n;
            read_grow(f, cent, ix->nlist * ix->dim);
            read_grow(f, cb, ix->ksub * ix->dim);
            read_list_offsets(f, *ix, PQ);
            read_grow(f, codes, ix->n * pq_file_row_bytes(ix->m, bits));
            expect_end(f);
            if (bits == 4 && ix->m % 2)
                for (size_t r = 0, fb = pq_file_row_bytes(ix->m, 4); r < ix->n; r++)
                    if (codes[r * fb + fb - 1] >> 4)
                        fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index: the pad nibble of row %zu is not zero", r);
            for (float v : cb)
                if (!std::isfinite(v))
                    fail(MSVS_ERR_IO, "corrupt msvs IVFPQ index: a codebook entry is not finite");
        }
        const std::vector<int64_t> ids = read_id_file(io, "pq_ids", "MSVSPQID", ix->n, PQ);
        // the stored form: code words in transposed blocks of 64 rows, labels as u32
        upload_centroids(*ix, cent.data(), ix->nlist, MSVS_MEM_HOST, stream);
        pq_set_codebooks(*ix, cb.data(), stream);
        alloc_lists(*ix, ix->n, 64, true, stream);
        const size_t fb = pq_file_row_bytes(ix->m, ix->bits);
        pq_each_piece(*ix, hipMemcpyHostToDevice, stream, [&](size_t r0, size_t cnt, uint32_t * words) {
            for (size_t r = 0; r < cnt; r++)
                for (size_t i = 0; i < fb; i++)
                    words[pq_code_word(r, (uint32_t)(i >> 2), ix->mw)] |= (uint32_t)codes[(r0 + r) * fb + i] << (8 * (i & 3));
        });
        finish_load(*ix, ids, stream);
        pq_compute_row_terms(*ix, stream);
        *out = ix.release();
    });
}
