// binary.hip -- seam A2 for BinaryVector: msvs_knn_bin[_rounds] (include/msvs.h), see bin_kernels.hpp; below it seam A1, the binary
// index (flat and partitioned), with host-pointer, device-pointer and rank-round (k > MSVS_MAX_K) entries.
#include <algorithm>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "bin_ivf_kernels.hpp"
#include "bin_kernels.hpp"
#include "device_ops.hpp"
#include "io_stream.hpp"
#include "list_layout.hpp"

namespace msvs
{

/// lanes per row: one 16-byte word each per step
static uint32_t bin_lanes(uint32_t ld16)
{
    uint32_t g = 1;
    while (g < 16 && g * 2 <= ld16)
        g *= 2;
    return g;
}

constexpr uint32_t BIN_IVF_T = 8;                     // queries per tile of the list scan (4 beyond k = 64)
constexpr size_t BIN_ASSIGN_LDS = (size_t)48 << 10;   // centroid tile of the assign kernel

/// rows (or queries) against the centroids: best[n] (list of the smallest (distance, id)) and / or dist[n][nlist].
static void launch_bin_assign(const unsigned char * dy, const unsigned char * dc, size_t n, size_t nlist, uint32_t ld16, uint32_t * best,
                              uint32_t * dist, hipStream_t stream)
{
    if (n == 0 || nlist == 0)
        return;
    ProfileScope prof("bin_ivf_coarse", stream);
    const uint32_t g = bin_lanes(ld16);
    BinAssignParams a{};
    a.Y = reinterpret_cast<const uint4 *>(dy);
    a.C = reinterpret_cast<const uint4 *>(dc);
    a.n = (uint32_t)n;
    a.nlist = (uint32_t)nlist;
    a.ld16 = ld16;
    a.tile = (uint32_t)std::max<size_t>(1, std::min(nlist, BIN_ASSIGN_LDS / ((size_t)ld16 * 16)));
    a.best = best;
    a.dist = dist;
    const dim3 grid((unsigned)ceil_div(n, (size_t)(BLOCK / g)));
    const size_t lds = (size_t)a.tile * ld16 * 16;
    with_int<1, 2, 4, 8, 16>(g, [&](auto lanes) {
        hipLaunchKernelGGL((bin_assign_kernel<decltype(lanes)::value>), grid, dim3(BLOCK), lds, stream, a);
    });
    MSVS_HIP(hipGetLastError());
}

/// g: lanes per row, a power of two up to 16 (bin_lanes).  A later rank round (a.after) takes the AFTER form, which exists with four
/// top-k registers per lane only: such a round follows one of MSVS_MAX_K ranks, and its own k is the search's remainder.
static void launch_bin_scan(int metric, uint32_t g, const BinParams & a, hipStream_t stream)
{
    ProfileScope prof("bin_scan", stream);
    const dim3 grid(a.n_blocks, a.nq);
    const size_t lds = (size_t)a.ld16 * 16 + (size_t)5 * a.k * 8;
    with_int<B_HAMMING, B_JACCARD>(metric == MSVS_METRIC_HAMMING ? B_HAMMING : B_JACCARD, [&](auto m) {
        with_int<1, 2, 4, 8, 16>(g, [&](auto lanes) {
            constexpr int METRIC = decltype(m)::value, G = decltype(lanes)::value;
            if (a.after)
                hipLaunchKernelGGL((bin_scan_kernel<METRIC, G, 4, 1>), grid, dim3(BLOCK), lds, stream, a);
            else
                with_int<1, 4>(a.k <= 64 ? 1 : 4, [&](auto r) {
                    hipLaunchKernelGGL((bin_scan_kernel<METRIC, G, decltype(r)::value>), grid, dim3(BLOCK), lds, stream, a);
                });
        });
    });
    MSVS_HIP(hipGetLastError());
}

/// queries per tile of the list scan for a plan whose (first) round returns k ranks
static uint32_t bin_ivf_tile(size_t k) { return k <= 64 ? BIN_IVF_T : BIN_IVF_T / 2; }

/// List scan over the plan's work items; tiles of BIN_IVF_T queries with one top-k register per lane up to k = 64, half the tile and
/// four registers beyond; REG: the row fits the group's registers (ld16 == G).  A later rank round (a.after) takes the AFTER form,
/// which exists in the second shape only: the plan it walks was made for a first round of MSVS_MAX_K ranks, whatever its own k.
static void launch_bin_ivf_scan(int metric, uint32_t g, uint32_t grid, const BinIvfParams & a, hipStream_t stream)
{
    ProfileScope prof("bin_ivf_scan", stream);
    with_int<B_HAMMING, B_JACCARD>(metric == MSVS_METRIC_HAMMING ? B_HAMMING : B_JACCARD, [&](auto m) {
        with_int<1, 2, 4, 8, 16>(g, [&](auto lanes) {
            with_bool(a.ld16 == (uint32_t)decltype(lanes)::value, [&](auto reg) {
                constexpr int METRIC = decltype(m)::value, G = decltype(lanes)::value;
                constexpr bool REG = decltype(reg)::value;
                if (a.after)
                {
                    constexpr int T = BIN_IVF_T / 2;
                    const size_t lds = (size_t)T * a.ld16 * 16 + (size_t)5 * a.k * 8;
                    hipLaunchKernelGGL((bin_ivf_scan_kernel<METRIC, G, T, 4, REG, 1>), dim3(grid), dim3(BLOCK), lds, stream, a);
                }
                else
                    with_bool(a.k <= 64, [&](auto small) {
                        constexpr int T = decltype(small)::value ? BIN_IVF_T : BIN_IVF_T / 2, R = decltype(small)::value ? 1 : 4;
                        const size_t lds = (size_t)T * a.ld16 * 16 + (size_t)5 * a.k * 8;
                        hipLaunchKernelGGL((bin_ivf_scan_kernel<METRIC, G, T, R, REG>), dim3(grid), dim3(BLOCK), lds, stream, a);
                    });
            });
        });
    });
    MSVS_HIP(hipGetLastError());
}

}

using namespace msvs;

// Both searches come as a device core (everything enqueued on `stream`: queries, filter and outputs are DEVICE pointers, nothing waits
// for the host) and a host-pointer wrapper around it (bin_search_host).  k > MSVS_MAX_K runs in rank rounds like the coded indexes'
// search_device (coded_ivf.hpp): everything up to the plan once per chunk of queries, then ceil(k / MSVS_MAX_K) times the scan with
// k_round = min(MSVS_MAX_K, k - done) ranks (from the second round on its AFTER form: only rows whose key is strictly greater than the
// query's continuation key), the merge to keys, and launch_round_scatter into columns [done, done + k_round) of the [nx][k] outputs,
// which also writes the continuation key -- a full round's last key, KEY_NONE after a short one.  Hamming distances are small
// integers: a round boundary nearly always falls inside a run of equal distances, and the label half of the key carries the
// continuation there.  Segments, tile, LDS and partial lists are sized by min(k, MSVS_MAX_K).

constexpr size_t BIN_FLAT_CHUNK = 65535; // queries of one flat scan launch (they sit on grid.y)

/// d_x: n dense rows of nbytes on the device -> n rows of ldb bytes (zero padded) in dq
static void bin_pad_device_rows(unsigned char * dq, const uint8_t * d_x, size_t n, size_t nbytes, size_t ldb, hipStream_t stream)
{
    if (ldb != nbytes)
        MSVS_HIP(hipMemsetAsync(dq, 0, n * ldb, stream));
    MSVS_HIP(hipMemcpy2DAsync(dq, ldb, d_x, nbytes, nbytes, n, hipMemcpyDeviceToDevice, stream));
}

/// The scan + merge over rows already on the device (dy: n rows of ldb bytes, zero padded to 16-byte words); d_x (nx dense rows of
/// nbytes), d_alive (over labels, nbits of them), d_ids, d_dis ([nx][k]) on the DEVICE.
static void bin_search_rows_device(const unsigned char * dy, const uint32_t * d_labels, size_t ny, size_t nbytes, const uint8_t * d_x, size_t nx,
                                   size_t k, int metric, const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis,
                                   hipStream_t stream)
{
    const uint32_t ld16 = (uint32_t)ceil_div(nbytes, (size_t)16);
    const size_t ldb = (size_t)ld16 * 16;
    const bool rounds = k > MSVS_MAX_K;
    const size_t kl = std::min<size_t>(k, MSVS_MAX_K); // ranks of one scan
    if (ldb + 5 * kl * 8 > SCAN_LDS_BUDGET)
        fail(MSVS_ERR_INVALID_ARGUMENT, "binary vectors of %zu bytes are too long for the LDS query stage", nbytes);
    const uint32_t g = bin_lanes(ld16);
    const size_t chunk = std::min(nx, BIN_FLAT_CHUNK);
    // row ranges: ~2048 blocks over the chip, at least one wavefront step each
    const size_t rows_step = 4 * (64 / g);
    const size_t want = std::max<size_t>(1, 2048 / chunk);
    const size_t nb = std::max<size_t>(1, std::min(want, ceil_div(std::max<size_t>(ny, 1), rows_step)));
    const uint32_t rpb = (uint32_t)round_up(ceil_div(std::max<size_t>(ny, 1), nb), rows_step);
    const uint32_t n_blocks = (uint32_t)ceil_div(std::max<size_t>(ny, 1), (size_t)rpb);
    Scratch & scr = scratch_for(stream);
    scr.reserve(chunk * ldb + chunk * (size_t)n_blocks * kl * 8 + (rounds ? chunk * (size_t)(MSVS_MAX_K + 1) * 8 : 0) + 8192, stream);
    unsigned char * dq = scr.take<unsigned char>(chunk * ldb);
    uint64_t * partial = scr.take<uint64_t>(chunk * (size_t)n_blocks * kl);
    uint64_t * round_keys = rounds ? scr.take<uint64_t>(chunk * MSVS_MAX_K) : nullptr;
    uint64_t * after = rounds ? scr.take<uint64_t>(chunk) : nullptr;
    for (size_t q0 = 0; q0 < nx; q0 += chunk)
    {
        const size_t nq = std::min(chunk, nx - q0);
        bin_pad_device_rows(dq, d_x + q0 * nbytes, nq, nbytes, ldb, stream);
        BinParams a{};
        a.Y = reinterpret_cast<const uint4 *>(dy);
        a.Q = reinterpret_cast<const uint4 *>(dq);
        a.alive = d_alive;
        a.labels = d_labels;
        a.nbits = (uint32_t)std::min<size_t>(nbits, 0xffffffffu);
        a.ld16 = ld16;
        a.n_rows = (uint32_t)ny;
        a.rows_per_block = rpb;
        a.n_blocks = n_blocks;
        a.nq = (uint32_t)nq;
        a.partial = partial;
        for (size_t done = 0; done < k; done += MSVS_MAX_K) // (one pass unless `rounds`)
        {
            const size_t kr = std::min<size_t>(MSVS_MAX_K, k - done);
            a.k = (uint32_t)kr;
            a.after = done ? after : nullptr;
            launch_bin_scan(metric, g, a, stream);
            MergeParams m{};
            m.partial = partial;
            m.n_lists = n_blocks;
            m.k = (uint32_t)kr;
            m.out_ids = d_ids + q0 * k;
            m.out_dis = d_dis + q0 * k;
            if (rounds)
            {
                m.mode = 2;
                m.out_keys = round_keys;
            }
            launch_merge(M_L2, m, (uint32_t)nq, stream);
            if (rounds)
                launch_round_scatter(M_L2, round_keys, nq, kr, k, done, false, d_ids + q0 * k, d_dis + q0 * k, after, stream);
        }
    }
}

/// The host-pointer form of a device core: the queries (nx dense rows of nbytes) and the filter staged to the device,
/// dev(d_x, d_alive, d_ids, d_dis) enqueues the search on `stream`, the results are copied back; synchronises.
template <class DeviceSearch>
static void bin_search_host(const uint8_t * x, size_t nx, size_t nbytes, size_t k, const uint64_t * alive_bits, size_t nbits, int64_t * ids,
                            float * dis, hipStream_t stream, DeviceSearch dev)
{
    const size_t words = alive_bits ? std::max<size_t>(1, ceil_div(nbits, (size_t)64)) : 0;
    Scratch & stg = staging_for(stream);
    stg.reserve(nx * nbytes + nx * k * 12 + words * 8 + 4 * 256, stream);
    unsigned char * d_x = stg.take<unsigned char>(nx * nbytes);
    int64_t * d_ids = stg.take<int64_t>(nx * k);
    float * d_dis = stg.take<float>(nx * k);
    uint64_t * d_alive = words ? stg.take<uint64_t>(words) : nullptr;
    MSVS_HIP(hipMemcpyAsync(d_x, x, nx * nbytes, hipMemcpyHostToDevice, stream));
    if (words)
        MSVS_HIP(hipMemcpyAsync(d_alive, alive_bits, words * 8, hipMemcpyHostToDevice, stream));
    dev(d_x, d_alive, d_ids, d_dis);
    MSVS_HIP(hipMemcpyAsync(ids, d_ids, nx * k * 8, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipMemcpyAsync(dis, d_dis, nx * k * 4, hipMemcpyDeviceToHost, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
}

/// k_max: the entry's limit of k (MSVS_MAX_K, or MSVS_MAX_K_ROUNDS for the entries that search in rank rounds)
static void bin_check_args(size_t nbytes, size_t k, int metric, size_t k_max = MSVS_MAX_K)
{
    if (metric != MSVS_METRIC_HAMMING && metric != MSVS_METRIC_JACCARD)
        fail(MSVS_ERR_NOT_IMPLEMENTED, "Metric not implemented in brute force search for Binary Vector");
    if (nbytes == 0)
        fail(MSVS_ERR_INVALID_ARGUMENT, "zero dimension");
    if (k > k_max)
        fail(MSVS_ERR_UNSUPPORTED_K, "k = %zu exceeds the device top-k limit %d", k, (int)k_max);
}

static void bin_knn(const uint8_t * x, const uint8_t * y, size_t nbytes, size_t k, size_t k_max, size_t nx, size_t ny, int metric,
                    const uint64_t * alive_bits, int64_t * ids, float * dis)
{
    bin_check_args(std::max<size_t>(nbytes, 1), k, metric, k_max);
    if (nx == 0 || k == 0)
        return;
    if (!x || !ids || !dis || (ny && !y) || nbytes == 0)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer or zero dimension");
    if (ny > 0xfffffff0ull)
        fail(MSVS_ERR_ID_RANGE, "ny exceeds the u32 id range");
    hipStream_t stream = thread_stream();
    const size_t ldb = round_up(nbytes, (size_t)16);
    DevBuf<unsigned char> dy(std::max<size_t>(ny, 1) * ldb);
    if (ldb != nbytes)
        MSVS_HIP(hipMemsetAsync(dy.p, 0, std::max<size_t>(ny, 1) * ldb, stream));
    if (ny)
        MSVS_HIP(hipMemcpy2DAsync(dy.p, ldb, y, nbytes, nbytes, ny, hipMemcpyHostToDevice, stream));
    bin_search_host(x, nx, nbytes, k, alive_bits, ny, ids, dis, stream,
                    [&](const uint8_t * d_x, const uint64_t * d_alive, int64_t * d_ids, float * d_dis) {
                        bin_search_rows_device(dy.p, nullptr, ny, nbytes, d_x, nx, k, metric, d_alive, ny, d_ids, d_dis, stream);
                    });
}

extern "C" int msvs_knn_bin(const uint8_t * x, const uint8_t * y, size_t nbytes, size_t k, size_t nx, size_t ny, int metric,
                            const uint64_t * alive_bits, int64_t * ids, float * dis)
{
    return guarded([&] { bin_knn(x, y, nbytes, k, MSVS_MAX_K, nx, ny, metric, alive_bits, ids, dis); });
}

extern "C" int msvs_knn_bin_rounds(const uint8_t * x, const uint8_t * y, size_t nbytes, size_t k, size_t nx, size_t ny, int metric,
                                   const uint64_t * alive_bits, int64_t * ids, float * dis)
{
    return guarded([&] { bin_knn(x, y, nbytes, k, MSVS_MAX_K_ROUNDS, nx, ny, metric, alive_bits, ids, dis); });
}

// ------------------------------------------------------------------------------------------- seam A1 for BinaryVector
//
// Search::VectorIndex<IS, OS, Bitmap, BinaryVector> (VICommon.h:142-143; created at VIWithDataPart.cpp:431-446, searched at
// :928-935): BinaryFLAT -- and the partition scan of BinaryMSTG, whose algorithm is not in the reference -- as an exhaustive
// scan of RESIDENT rows: the part's FixedString(N) column is uploaded once at build / load, a search sends the query bits and
// the filter bitmap.  Labels are the part's row offsets (what VIPartReader hands out as ids); the filter is indexed by label.

struct msvs_bin_index
{
    size_t nbytes = 0;
    int metric = MSVS_METRIC_HAMMING;
    std::vector<uint8_t> rows;   // host copy: n x nbytes (the serialised form), insertion order
    std::vector<int64_t> labels; // n
    // the partitioned form (msvs_bin_index_create_ivf): ncentroids > 0; the centroids come from train / set_centroids / load
    size_t ncentroids = 0;          // 0: the flat index
    int niter = 10;                 // rounds of majority Lloyd in train
    std::vector<uint8_t> centroids; // ncentroids x nbytes, empty until the index is ready
    mutable std::mutex mu;
    /// The rows as a search reads them, on ONE device: n x round_up(nbytes, 16) + labels, uploaded at the first search (on that
    /// device) after an add.  Searches hold the image through a shared_ptr while they scan: an add that comes in meanwhile
    /// replaces the map entry, the buffers go when the last scan that uses them is done.
    /// Partitioned: the rows are LIST-MAJOR (list = smallest (Hamming distance to the centroid, list id), assigned on the device;
    /// ascending label inside a list), rebuilt from the centroids here -- the host copy and the files stay in insertion order.
    struct Image
    {
        DevBuf<unsigned char> rows;
        DevBuf<uint32_t> labels;
        size_t n = 0;
        DevBuf<unsigned char> cent;  // nlist x round_up(nbytes, 16)
        DevBuf<int64_t> list_off;    // nlist + 1
        std::vector<int64_t> h_off;  // the same on the host
        std::vector<uint32_t> perm;  // storage position -> insertion position
        size_t nlist = 0, max_len = 0;
    };
    mutable std::map<int, std::shared_ptr<Image>> images; // by device; cleared by add
    bool partitioned() const { return ncentroids != 0; }
    bool ready() const { return !partitioned() || !centroids.empty(); }
};

/// n host rows of nbytes -> n device rows of ldb bytes (zero padded)
static void bin_upload_padded(unsigned char * d, const uint8_t * h, size_t n, size_t nbytes, size_t ldb, hipStream_t stream)
{
    if (n == 0)
        return;
    if (ldb != nbytes)
        MSVS_HIP(hipMemsetAsync(d, 0, n * ldb, stream));
    MSVS_HIP(hipMemcpy2DAsync(d, ldb, h, nbytes, nbytes, n, hipMemcpyHostToDevice, stream));
}

/// The image of the calling thread's device, built if an add (or new centroids) dropped it.
static std::shared_ptr<msvs_bin_index::Image> bin_image(const msvs_bin_index * ix, hipStream_t stream)
{
    const size_t ldb = round_up(ix->nbytes, (size_t)16);
    int dev = 0;
    MSVS_HIP(hipGetDevice(&dev));
    // the row count is read and the upload made under ONE lock: an add between the two would otherwise leave rows that
    // are never searched; the image is per device (a search thread bound to another GPU gets its own copy)
    std::lock_guard<std::mutex> lk(ix->mu);
    auto & slot = ix->images[dev];
    if (slot)
        return slot;
    const size_t n = ix->labels.size();
    auto fresh = std::make_shared<msvs_bin_index::Image>();
    fresh->n = n;
    fresh->rows.alloc(std::max<size_t>(n, 1) * ldb);
    fresh->labels.alloc(std::max<size_t>(n, 1));
    MSVS_HIP(hipMemsetAsync(fresh->rows.p, 0, std::max<size_t>(n, 1) * ldb, stream));
    std::vector<uint32_t> l32(std::max<size_t>(n, 1));
    if (!ix->partitioned())
    {
        if (n)
        {
            MSVS_HIP(hipMemcpy2DAsync(fresh->rows.p, ldb, ix->rows.data(), ix->nbytes, ix->nbytes, n, hipMemcpyHostToDevice, stream));
            for (size_t i = 0; i < n; i++)
                l32[i] = (uint32_t)ix->labels[i];
            MSVS_HIP(hipMemcpyAsync(fresh->labels.p, l32.data(), n * 4, hipMemcpyHostToDevice, stream));
        }
        MSVS_HIP(hipStreamSynchronize(stream)); // l32 is about to go
        slot = fresh;
        return slot;
    }
    if (!ix->ready())
        fail(MSVS_ERR_NOT_READY, "the partitioned binary index has no centroids yet");
    const size_t nlist = ix->ncentroids;
    fresh->nlist = nlist;
    fresh->cent.alloc(nlist * ldb);
    fresh->list_off.alloc(nlist + 1);
    fresh->h_off.assign(nlist + 1, 0);
    fresh->perm.resize(n);
    MSVS_HIP(hipMemsetAsync(fresh->cent.p, 0, nlist * ldb, stream));
    bin_upload_padded(fresh->cent.p, ix->centroids.data(), nlist, ix->nbytes, ldb, stream);
    if (n)
    {
        // exact assignment on the device over the rows in insertion order (they sit in the image's own buffer for that), ...
        std::vector<uint32_t> list(n);
        {
            DevBuf<uint32_t> d_best(n);
            MSVS_HIP(hipMemcpy2DAsync(fresh->rows.p, ldb, ix->rows.data(), ix->nbytes, ix->nbytes, n, hipMemcpyHostToDevice, stream));
            launch_bin_assign(fresh->rows.p, fresh->cent.p, n, nlist, (uint32_t)(ldb / 16), d_best.p, nullptr, stream);
            MSVS_HIP(hipMemcpyAsync(list.data(), d_best.p, n * 4, hipMemcpyDeviceToHost, stream));
            MSVS_HIP(hipStreamSynchronize(stream));
        }
        // ... then list-major by (list, label, insertion position) on the host, and the permuted rows go up
        for (size_t i = 0; i < n; i++)
        {
            if (list[i] >= nlist)
                fail(MSVS_ERR_DEVICE, "internal: row %zu was assigned to list %u of %zu", i, list[i], nlist);
            l32[i] = (uint32_t)ix->labels[i];
        }
        ListLayout lay = list_major_layout(list.data(), l32.data(), n, nlist);
        fresh->h_off = std::move(lay.list_off);
        fresh->max_len = lay.max_list_len;
        fresh->perm = std::move(lay.order);
        std::vector<uint8_t> lm(n * ldb, 0);
        for (size_t i = 0; i < n; i++)
        {
            const uint32_t src = fresh->perm[i];
            l32[i] = (uint32_t)ix->labels[src];
            memcpy(lm.data() + i * ldb, ix->rows.data() + (size_t)src * ix->nbytes, ix->nbytes);
        }
        MSVS_HIP(hipMemcpyAsync(fresh->rows.p, lm.data(), n * ldb, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipMemcpyAsync(fresh->labels.p, l32.data(), n * 4, hipMemcpyHostToDevice, stream));
        MSVS_HIP(hipStreamSynchronize(stream)); // lm, l32 are about to go
    }
    MSVS_HIP(hipMemcpyAsync(fresh->list_off.p, fresh->h_off.data(), (nlist + 1) * 8, hipMemcpyHostToDevice, stream));
    MSVS_HIP(hipStreamSynchronize(stream));
    slot = fresh;
    return slot;
}

/// Coarse probe, plan, list scan and merge over a partitioned image; d_x, d_alive, d_ids, d_dis on the DEVICE (as bin_search_rows_device).
static void bin_ivf_search_image_device(const msvs_bin_index::Image & img, size_t nbytes, int metric, const uint8_t * d_x, size_t nx, size_t k,
                                        size_t nprobe, const uint64_t * d_alive, size_t nbits, int64_t * d_ids, float * d_dis,
                                        hipStream_t stream)
{
    const uint32_t ld16 = (uint32_t)ceil_div(nbytes, (size_t)16);
    const size_t ldb = (size_t)ld16 * 16;
    const uint32_t g = bin_lanes(ld16);
    const size_t nlist = img.nlist, P = std::min(nprobe, nlist);
    const bool rounds = k > MSVS_MAX_K;
    const size_t kl = std::min<size_t>(k, MSVS_MAX_K); // ranks of one scan
    // row segments of whole wavefront steps; per query of a round: its distances to the centroids, probes and pairs, padded row
    // (rounds: a round's merged keys and the continuation key)
    const SegmentPlan sp = plan_segments(img.max_len, options().bin_ivf_rpb, 4 * (64 / g), P, kl,
                                         nlist * 4 + P * 8 + ldb + (rounds ? (size_t)(MSVS_MAX_K + 1) * 8 : 0), nx);
    const uint32_t rpb = sp.rpb;
    const size_t seg_max = sp.seg_max, per_q = sp.per_q, chunk = sp.chunk;
    Scratch & scr = scratch_for(stream);
    scr.reserve(chunk * per_q + (nlist + 1) * 16 + 16 * 256, stream);
    unsigned char * dq = scr.take<unsigned char>(chunk * ldb);
    uint32_t * dist = scr.take<uint32_t>(chunk * nlist);
    int32_t * probes = scr.take<int32_t>(chunk * P);
    const GroupedPlan plan(scr, nlist, chunk * P);
    uint64_t * partial = scr.take<uint64_t>(chunk * P * seg_max * kl);
    uint64_t * round_keys = rounds ? scr.take<uint64_t>(chunk * MSVS_MAX_K) : nullptr;
    uint64_t * after = rounds ? scr.take<uint64_t>(chunk) : nullptr;
    for (size_t q0 = 0; q0 < nx; q0 += chunk)
    {
        const size_t nq = std::min(chunk, nx - q0);
        bin_pad_device_rows(dq, d_x + q0 * nbytes, nq, nbytes, ldb, stream);
        launch_bin_assign(dq, img.cent.p, nq, nlist, ld16, nullptr, dist, stream);
        hipLaunchKernelGGL(bin_probe_select_kernel, dim3((unsigned)nq), dim3(BLOCK), 0, stream, dist, (uint32_t)nlist, (uint32_t)P, ld16 * 128u, probes);
        MSVS_HIP(hipGetLastError());
        plan.run(probes, img.list_off.p, nq * P, rpb, bin_ivf_tile(kl), stream);
        BinIvfParams a{};
        a.Y = reinterpret_cast<const uint4 *>(img.rows.p);
        a.Q = reinterpret_cast<const uint4 *>(dq);
        a.alive = d_alive;
        a.labels = img.labels.p;
        a.nbits = (uint32_t)std::min<size_t>(nbits, 0xffffffffu);
        a.ld16 = ld16;
        a.nprobe = (uint32_t)P;
        a.nlist = (uint32_t)nlist;
        a.rows_per_block = rpb;
        a.seg_max = (uint32_t)seg_max;
        a.list_off = img.list_off.p;
        a.pair_off = plan.pair_off;
        a.work_off = plan.work_off;
        a.pairs = plan.pairs;
        a.partial = partial;
        for (size_t done = 0; done < k; done += MSVS_MAX_K) // (one pass unless `rounds`)
        {
            const size_t kr = std::min<size_t>(MSVS_MAX_K, k - done);
            a.k = (uint32_t)kr;
            a.after = done ? after : nullptr;
            // KEY_NONE: (pair, segment) slots without rows -- every round anew, the slots of a round are k_round keys apart
            MSVS_HIP(hipMemsetAsync(partial, 0xff, nq * P * seg_max * kr * 8, stream));
            launch_bin_ivf_scan(metric, g, (uint32_t)std::min<size_t>(2048, nq * P * seg_max), a, stream);
            MergeParams m{};
            m.partial = partial;
            m.n_lists = (uint32_t)(P * seg_max);
            m.k = (uint32_t)kr;
            m.out_ids = d_ids + q0 * k;
            m.out_dis = d_dis + q0 * k;
            if (rounds)
            {
                m.mode = 2;
                m.out_keys = round_keys;
            }
            launch_merge(M_L2, m, (uint32_t)nq, stream);
            if (rounds)
                launch_round_scatter(M_L2, round_keys, nq, kr, k, done, false, d_ids + q0 * k, d_dis + q0 * k, after, stream);
        }
    }
}

extern "C" int msvs_bin_index_create(size_t nbytes, int metric, msvs_bin_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        bin_check_args(nbytes, 1, metric);
        std::unique_ptr<msvs_bin_index> ix(new msvs_bin_index);
        ix->nbytes = nbytes;
        ix->metric = metric;
        *out = ix.release();
    });
}

/// what the list scan's LDS stage holds: a tile of queries + the merge lists of the largest k
static bool bin_ivf_fits(size_t nbytes)
{
    return BIN_IVF_T * round_up(nbytes, (size_t)16) + (size_t)5 * MSVS_MAX_K * 8 <= SCAN_LDS_BUDGET;
}

extern "C" int msvs_bin_index_create_ivf(size_t nbytes, int metric, const char * params, msvs_bin_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        *out = nullptr;
        bin_check_args(nbytes, 1, metric);
        if (!bin_ivf_fits(nbytes))
            fail(MSVS_ERR_INVALID_ARGUMENT, "binary vectors of %zu bytes are too long for the partitioned index", nbytes);
        auto p = parse_params(params);
        const long nc = param_int(p, "ncentroids", 1024), niter = param_int(p, "niter", 10);
        if (nc < 1 || nc > 0x7fffffffl || niter < 0)
            fail(MSVS_ERR_INVALID_ARGUMENT, "bad ncentroids / niter");
        std::unique_ptr<msvs_bin_index> ix(new msvs_bin_index);
        ix->nbytes = nbytes;
        ix->metric = metric;
        ix->ncentroids = (size_t)nc;
        ix->niter = (int)niter;
        *out = ix.release();
    });
}

extern "C" void msvs_bin_index_free(msvs_bin_index_t * ix) { delete ix; }

extern "C" size_t msvs_bin_index_num_lists(const msvs_bin_index_t * ix) { return ix ? ix->ncentroids : 0; }

extern "C" int msvs_bin_index_set_centroids(msvs_bin_index_t * ix, const uint8_t * centroids, size_t nlist)
{
    return guarded([&] {
        if (!ix || !centroids)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / centroids");
        if (!ix->partitioned() || nlist != ix->ncentroids)
            fail(MSVS_ERR_INVALID_ARGUMENT, "%zu centroids given, the index has ncentroids = %zu", nlist, ix->ncentroids);
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->centroids.assign(centroids, centroids + nlist * ix->nbytes);
        ix->images.clear(); // the lists are rebuilt from the new centroids at the next search
    });
}

extern "C" int msvs_bin_index_train(msvs_bin_index_t * ix, const uint8_t * rows, size_t n)
{
    return guarded([&] {
        if (!ix || (n && !rows))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / rows");
        if (!ix->partitioned())
            fail(MSVS_ERR_INVALID_ARGUMENT, "a flat binary index is not trained");
        const size_t nlist = ix->ncentroids, nbytes = ix->nbytes;
        if (n < nlist)
            fail(MSVS_ERR_INVALID_ARGUMENT, "%zu training rows for %zu centroids", n, nlist);
        if (n > 0xfffffff0ull)
            fail(MSVS_ERR_ID_RANGE, "more training rows than the u32 range");
        // seeds: rows at fixed, evenly spaced positions (no RNG: the same input trains the same centroids)
        std::vector<uint8_t> cent(nlist * nbytes);
        for (size_t l = 0; l < nlist; l++)
            memcpy(cent.data() + l * nbytes, rows + (l * n / nlist) * nbytes, nbytes);
        if (ix->niter > 0)
        {
            hipStream_t stream = thread_stream();
            const size_t ldb = round_up(nbytes, (size_t)16);
            const uint32_t ld16 = (uint32_t)(ldb / 16), words = ld16 * 4;
            DevBuf<unsigned char> dy(n * ldb), dc(nlist * ldb);
            DevBuf<uint32_t> d_list(n), d_votes(nlist * (size_t)words * 32 + nlist);
            uint32_t * d_ones = d_votes.p, * d_members = d_votes.p + nlist * (size_t)words * 32;
            std::vector<uint32_t> votes(d_votes.n);
            MSVS_HIP(hipMemsetAsync(dc.p, 0, nlist * ldb, stream));
            bin_upload_padded(dy.p, rows, n, nbytes, ldb, stream);
            for (int it = 0; it < ix->niter; it++)
            {
                // exact assignment and the per-bit vote counts on the device, the majority (2 * ones > members) here
                bin_upload_padded(dc.p, cent.data(), nlist, nbytes, ldb, stream);
                launch_bin_assign(dy.p, dc.p, n, nlist, ld16, d_list.p, nullptr, stream);
                MSVS_HIP(hipMemsetAsync(d_votes.p, 0, d_votes.bytes(), stream));
                {
                    ProfileScope prof("bin_ivf_vote", stream);
                    const size_t threads = n * words;
                    hipLaunchKernelGGL(bin_vote_kernel, dim3((unsigned)ceil_div(threads, (size_t)256)), dim3(256), 0, stream,
                                       reinterpret_cast<const uint32_t *>(dy.p), d_list.p, n, words, d_ones, d_members);
                    MSVS_HIP(hipGetLastError());
                }
                MSVS_HIP(hipMemcpyAsync(votes.data(), d_votes.p, d_votes.bytes(), hipMemcpyDeviceToHost, stream));
                MSVS_HIP(hipStreamSynchronize(stream));
                const uint32_t * members = votes.data() + nlist * (size_t)words * 32;
                bool changed = false;
                for (size_t l = 0; l < nlist; l++)
                {
                    if (members[l] == 0)
                        continue; // an empty list keeps its centroid
                    const uint32_t * ones = votes.data() + l * (size_t)words * 32;
                    for (size_t b = 0; b < nbytes; b++)
                    {
                        uint8_t v = 0;
                        for (int bit = 0; bit < 8; bit++)
                            if (2 * (uint64_t)ones[b * 8 + bit] > members[l])
                                v |= (uint8_t)(1u << bit);
                        changed |= v != cent[l * nbytes + b];
                        cent[l * nbytes + b] = v;
                    }
                }
                if (!changed)
                    break; // a fixed point: further rounds repeat it
            }
        }
        std::lock_guard<std::mutex> lk(ix->mu);
        ix->centroids.swap(cent);
        ix->images.clear();
    });
}

extern "C" int msvs_bin_index_add(msvs_bin_index_t * ix, const uint8_t * rows, const int64_t * ids, size_t n)
{
    return guarded([&] {
        if (!ix || (n && !rows))
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index / rows");
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->ready())
            fail(MSVS_ERR_NOT_READY, "the partitioned binary index has no centroids yet (train / set_centroids)");
        const size_t base = ix->labels.size();
        if (base + n > 0xfffffff0ull)
            fail(MSVS_ERR_ID_RANGE, "more rows than the u32 label range");
        for (size_t i = 0; i < n; i++)
        {
            const int64_t id = ids ? ids[i] : (int64_t)(base + i);
            if (id < 0 || id > 0xfffffff0ll)
                fail(MSVS_ERR_ID_RANGE, "id %lld does not fit the u32 label range", (long long)id);
        }
        for (size_t i = 0; i < n; i++)
            ix->labels.push_back(ids ? ids[i] : (int64_t)(base + i));
        ix->rows.insert(ix->rows.end(), rows, rows + n * ix->nbytes);
        ix->images.clear(); // (scans in flight keep theirs alive)
    });
}

extern "C" size_t msvs_bin_index_num_data(const msvs_bin_index_t * ix) { return ix ? ix->labels.size() : 0; }

/// What every index search checks before it touches the device, in this order; false: nothing to do (nx or k is 0).
/// x, ids, dis: the entry's own pointers, host or device.
static bool bin_index_search_checks(const msvs_bin_index_t * ix, const void * x, size_t nx, size_t k, size_t k_max, size_t nprobe, const void * ids,
                                    const void * dis)
{
    if (!ix)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
    bin_check_args(ix->nbytes, k, ix->metric, k_max);
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        if (!ix->ready())
            fail(MSVS_ERR_NOT_READY, "the partitioned binary index has no centroids yet (train / set_centroids)");
    }
    if (ix->partitioned() && nprobe < 1)
        fail(MSVS_ERR_INVALID_ARGUMENT, "nprobe must be >= 1");
    if (nx == 0 || k == 0)
        return false;
    if (!x || !ids || !dis)
        fail(MSVS_ERR_INVALID_ARGUMENT, "null buffer");
    return true;
}

/// The device core of an index search (checked arguments, device pointers): the image of the calling thread's device -- built on
/// `stream`, with host synchronisation, if an add dropped it -- and the family's scan, enqueued on `stream`.
static void bin_index_search_device(const msvs_bin_index_t * ix, const uint8_t * d_x, size_t nx, size_t k, size_t nprobe, const uint64_t * d_alive,
                                    size_t nbits, int64_t * d_ids, float * d_dis, hipStream_t stream)
{
    const std::shared_ptr<msvs_bin_index::Image> img = bin_image(ix, stream);
    if (ix->partitioned())
        bin_ivf_search_image_device(*img, ix->nbytes, ix->metric, d_x, nx, k, nprobe, d_alive, nbits, d_ids, d_dis, stream);
    else
        bin_search_rows_device(img->rows.p, img->labels.p, img->n, ix->nbytes, d_x, nx, k, ix->metric, d_alive, nbits, d_ids, d_dis, stream);
}

// The C entries come in two forms that differ in their limit of k alone: the one-round form (k <= MSVS_MAX_K) and the rounds form
// (k <= MSVS_MAX_K_ROUNDS).

static int bin_index_search_entry(const msvs_bin_index_t * ix, const uint8_t * x, size_t nx, size_t k, size_t k_max, const char * params,
                                  const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return guarded([&] {
        const size_t nprobe = parse_nprobe(params);
        if (!bin_index_search_checks(ix, x, nx, k, k_max, nprobe, ids, dis))
            return;
        hipStream_t stream = thread_stream();
        bin_search_host(x, nx, ix->nbytes, k, alive_bits, nbits, ids, dis, stream,
                        [&](const uint8_t * d_x, const uint64_t * d_alive, int64_t * d_ids, float * d_dis) {
                            bin_index_search_device(ix, d_x, nx, k, nprobe, d_alive, nbits, d_ids, d_dis, stream);
                        });
    });
}

static int bin_index_search_device_entry(const msvs_bin_index_t * ix, const uint8_t * d_x, size_t nx, size_t k, size_t k_max, size_t nprobe,
                                         const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return guarded([&] {
        if (!bin_index_search_checks(ix, d_x, nx, k, k_max, nprobe, d_ids, d_dis))
            return;
        bin_index_search_device(ix, d_x, nx, k, nprobe, d_alive_bits, nbits, d_ids, d_dis, reinterpret_cast<hipStream_t>(hip_stream));
    });
}

extern "C" int msvs_bin_index_search(const msvs_bin_index_t * ix, const uint8_t * x, size_t nx, size_t k, const uint64_t * alive_bits,
                                     size_t nbits, int64_t * ids, float * dis)
{
    return bin_index_search_entry(ix, x, nx, k, MSVS_MAX_K, nullptr, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_bin_index_search_params(const msvs_bin_index_t * ix, const uint8_t * x, size_t nx, size_t k, const char * params,
                                            const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return bin_index_search_entry(ix, x, nx, k, MSVS_MAX_K, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_bin_index_search_rounds(const msvs_bin_index_t * ix, const uint8_t * x, size_t nx, size_t k, const char * params,
                                            const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis)
{
    return bin_index_search_entry(ix, x, nx, k, MSVS_MAX_K_ROUNDS, params, alive_bits, nbits, ids, dis);
}

extern "C" int msvs_bin_index_search_device(const msvs_bin_index_t * ix, const uint8_t * d_x, size_t nx, size_t k, size_t nprobe,
                                            const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream)
{
    return bin_index_search_device_entry(ix, d_x, nx, k, MSVS_MAX_K, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_bin_index_search_rounds_device(const msvs_bin_index_t * ix, const uint8_t * d_x, size_t nx, size_t k, size_t nprobe,
                                                   const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                   void * hip_stream)
{
    return bin_index_search_device_entry(ix, d_x, nx, k, MSVS_MAX_K_ROUNDS, nprobe, d_alive_bits, nbits, d_ids, d_dis, hip_stream);
}

extern "C" int msvs_bin_index_export(const msvs_bin_index_t * ix, uint8_t * centroids, int64_t * list_off, uint8_t * rows, int64_t * labels)
{
    return guarded([&] {
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        if (!ix->partitioned())
            fail(MSVS_ERR_INVALID_ARGUMENT, "a flat binary index has no lists to export");
        // (the image holds the list structure: it is built here if no search has done so since the last add)
        const std::shared_ptr<msvs_bin_index::Image> img = bin_image(ix, thread_stream());
        std::lock_guard<std::mutex> lk(ix->mu);
        if (img->n > ix->labels.size() || ix->centroids.size() != img->nlist * ix->nbytes)
            fail(MSVS_ERR_INVALID_ARGUMENT, "the index changed during the export");
        if (centroids)
            memcpy(centroids, ix->centroids.data(), ix->centroids.size());
        if (list_off)
            memcpy(list_off, img->h_off.data(), (img->nlist + 1) * 8);
        for (size_t i = 0; i < img->n; i++)
        {
            const size_t src = img->perm[i];
            if (rows)
                memcpy(rows + i * ix->nbytes, ix->rows.data() + src * ix->nbytes, ix->nbytes);
            if (labels)
                labels[i] = ix->labels[src];
        }
    });
}

namespace
{
struct BinHeader // 48 bytes, little endian
{
    char magic[8]; // "MSVSBIN1"
    uint32_t version; // 1: flat; 2: partitioned -- nlist / ncent below, the centroids after the rows
    int32_t metric;
    uint64_t nbytes, n;
    uint64_t nlist; // version 2: ncentroids (version 1: reserved, 0)
    uint64_t ncent; // version 2: centroids in the file, 0 (not trained yet) or nlist (version 1: reserved, 0)
};
}

extern "C" int msvs_bin_index_serialize_io(const msvs_bin_index_t * ix, const msvs_io_t * io)
{
    return guarded([&] {
        if (!ix)
            fail(MSVS_ERR_INVALID_ARGUMENT, "null index");
        std::lock_guard<std::mutex> lk(ix->mu);
        {
            IoStream f(io, "data_bin", 1);
            BinHeader h{};
            memcpy(h.magic, "MSVSBIN1", 8);
            h.version = ix->partitioned() ? 2 : 1;
            h.metric = ix->metric;
            h.nbytes = ix->nbytes;
            h.n = ix->labels.size();
            h.nlist = ix->ncentroids;
            h.ncent = ix->centroids.size() / ix->nbytes;
            f.write(&h, sizeof(h));
            if (!ix->rows.empty())
                f.write(ix->rows.data(), ix->rows.size());
            if (!ix->centroids.empty())
                f.write(ix->centroids.data(), ix->centroids.size());
            f.finish();
        }
        {
            IoStream f(io, "id_list", 1);
            const uint64_t n = ix->labels.size();
            f.write(&n, 8);
            if (n)
                f.write(ix->labels.data(), n * 8);
            f.finish();
        }
    });
}

extern "C" int msvs_bin_index_load_io(const msvs_io_t * io, msvs_bin_index_t ** out)
{
    return guarded([&] {
        if (!out)
            fail(MSVS_ERR_INVALID_ARGUMENT, "out is null");
        std::unique_ptr<msvs_bin_index> ix(new msvs_bin_index);
        {
            IoStream f(io, "data_bin", 0);
            BinHeader h{};
            f.read(&h, sizeof(h));
            if (memcmp(h.magic, "MSVSBIN1", 8) != 0 || (h.version != 1 && h.version != 2) || h.nbytes == 0 || h.nbytes > 65536
                || h.n > 0xfffffff0ull || (h.metric != MSVS_METRIC_HAMMING && h.metric != MSVS_METRIC_JACCARD))
                fail(MSVS_ERR_IO, "corrupt msvs binary index header");
            if (h.version == 2 && (h.nlist == 0 || h.nlist > 0x7fffffffull || (h.ncent != 0 && h.ncent != h.nlist) || !bin_ivf_fits(h.nbytes)))
                fail(MSVS_ERR_IO, "corrupt msvs binary index header (lists)");
            ix->nbytes = h.nbytes;
            ix->metric = h.metric;
            // the header is untrusted: the rows arrive in pieces and the buffer grows with what has really been read, so a corrupt
            // or truncated file ends in MSVS_ERR_IO (a short read) instead of a 2.8e14-byte allocation
            if (h.nbytes != 0 && h.n > SIZE_MAX / h.nbytes) // (n <= 0xfffffff0 and nbytes <= 65536 above: cannot wrap in 64 bits -- kept explicit)
                fail(MSVS_ERR_IO, "corrupt msvs binary index header");
            read_grow(f, ix->rows, (size_t)h.n * (size_t)h.nbytes);
            if (h.version == 2)
            {
                ix->ncentroids = (size_t)h.nlist;
                read_grow(f, ix->centroids, (size_t)h.ncent * (size_t)h.nbytes); // (< 2^31 * 2^16)
            }
            // (the labels are sized by the id list's own count below, piece by piece like the rows -- not by the header)
        }
        {
            IoStream f(io, "id_list", 0);
            uint64_t n = 0;
            f.read(&n, 8);
            const size_t rows_read = ix->nbytes ? ix->rows.size() / ix->nbytes : 0;
            if (n != rows_read)
                fail(MSVS_ERR_IO, "corrupt msvs binary index: %llu ids for %zu rows", (unsigned long long)n, rows_read);
            read_grow(f, ix->labels, (size_t)n); // in pieces, like the rows: the buffer grows with what has really been read
            for (int64_t id : ix->labels)
                if (id < 0 || id > 0xfffffff0ll)
                    fail(MSVS_ERR_IO, "corrupt msvs binary index: row id %lld outside the u32 row-offset range", (long long)id);
        }
        *out = ix.release();
    });
}
