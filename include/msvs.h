/*
 * msvs.h -- C-ABI of libmsvs.so: the MI355X (gfx950) vector-scan / BM25 hot path for MyScaleDB.
 *
 * Plain pointers and sizes only.  Every entry point replaces one call the MyScaleDB host makes
 * into its (absent) native libraries; the reference call site is cited at each declaration
 * (paths relative to the MyScaleDB tree).  INTEGRATION.md shows the host-side shims.
 *
 * Conventions kept from the reference:
 *   - ids are int64 row offsets local to the data part, -1 = "no result" (host tests `> -1`,
 *     src/VectorIndex/Storages/MergeTreeVSManager.cpp:1507,1523); on the device they must fit u32
 *     (the host stores labels in ColumnUInt32, MergeTreeVSManager.cpp:418-420);
 *   - results are sorted best-first; L2 is the SQUARED distance; cosine is 1 - <x^,y^>;
 *     IP is the raw dot product, larger is better;
 *   - unfilled slots carry the heap's neutral value: +FLT_MAX (L2), -FLT_MAX (IP),
 *     1 - (-FLT_MAX) (cosine, like VIWithDataPart.h:374-380);
 *   - ties are broken by ascending id (the reference leaves this to Faiss' heap);
 *   - filter bitmaps are LSB-first uint64 words, bit i of word i/64 <=> id i, 1 = candidate
 *     (the shim converts Search::DenseBitmap through is_member()/to_vector()).
 *
 * Threading: every function may be called concurrently from many host threads (the reference
 * allows 2 x cores concurrent searches, ScanThreadLimiter.h); index search is re-entrant on a
 * shared immutable index.  Errors: return value != MSVS_OK and a thread-local message in
 * msvs_last_error() -- the shim rethrows it as VIException (VICommon.h:75-104) so the host's
 * existing fallback logic applies.  There is NO CPU fallback inside this library.
 */
#ifndef MSVS_H
#define MSVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSVS_API __attribute__((visibility("default")))

typedef enum msvs_status {
    MSVS_OK = 0,
    MSVS_ERR_INVALID_ARGUMENT = 1,
    MSVS_ERR_NOT_IMPLEMENTED = 2, /* DB::ErrorCodes::NOT_IMPLEMENTED, BruteForceSearch.h:89-92 */
    MSVS_ERR_DEVICE = 3,          /* HIP runtime error; message carries hipGetErrorString */
    MSVS_ERR_OUT_OF_MEMORY = 4,
    MSVS_ERR_NOT_READY = 5, /* index->ready() == false, VIWithDataPart.cpp:876-879 */
    MSVS_ERR_UNSUPPORTED_K = 6,
    MSVS_ERR_ID_RANGE = 7,
    MSVS_ERR_IO = 8,
    MSVS_ERR_ABORTED = 236 /* = DB::ErrorCodes::ABORTED (src/Common/ErrorCodes.cpp: M(236, ABORTED)): the build was cancelled
                              through msvs_index_set_cancel -- what the host itself throws at VIPartReader.h:175-176 */
} msvs_status;

enum msvs_metric { MSVS_METRIC_L2 = 0, MSVS_METRIC_IP = 1, MSVS_METRIC_COSINE = 2, MSVS_METRIC_HAMMING = 3, MSVS_METRIC_JACCARD = 4 };
enum msvs_index_type { MSVS_INDEX_FLAT = 0, MSVS_INDEX_IVFFLAT = 1 };
enum msvs_mem { MSVS_MEM_HOST = 0, MSVS_MEM_DEVICE = 1 };

/* largest k (and nprobe) one device top-k pass supports; the limit of the sharded and routed searches and of every entry that has a
 * *_rounds twin (the coded and the binary indexes, msvs_knn_bin) */
#define MSVS_MAX_K 256
/* largest k of msvs_index_search[_filter][_device], msvs_knn_f32, the *_rounds entries, the BM25 entries and msvs_hybrid_fuse_device: beyond
 * MSVS_MAX_K they run exact rounds of MSVS_MAX_K ranks, each excluding the rows already returned (covers the reference's
 * k + deleted-rows over-fetch, LIMIT 1000 and the 3 x LIMIT candidates of a hybrid search).  The vector searches run their
 * rounds one query at a time; the BM25 entries over the whole batch at once.  Beyond it: MSVS_ERR_UNSUPPORTED_K. */
#define MSVS_MAX_K_ROUNDS 4096

MSVS_API const char * msvs_last_error(void);
MSVS_API const char * msvs_version(void);
MSVS_API int msvs_device_count(int * count);
MSVS_API int msvs_set_device(int ordinal);
MSVS_API int msvs_device_synchronize(void);

/* ---------------------------------------------------------------------------------------------
 * Seam A2 -- brute force.  Replaces the body of
 *   VectorIndex::tryBruteForceSearch<FloatVector>(x, y, d, k, nx, ny, result_id, distance, metric)
 *   (src/VectorIndex/Common/BruteForceSearch.h:63-92) = faiss::knn_L2sqr / faiss::knn_inner_product.
 * x: nx*d queries, y: ny*d base rows (row-major f32, HOST pointers); ids/dis: nx*k, caller-owned.
 * metric: MSVS_METRIC_L2 or MSVS_METRIC_IP; anything else -> MSVS_ERR_NOT_IMPLEMENTED like the
 * reference (cosine is composed above this call by searchWithoutIndex, VIWithDataPart.h:341-382).
 */
MSVS_API int msvs_knn_f32(const float * x, const float * y, size_t d, size_t k, size_t nx, size_t ny, int metric,
                          int64_t * ids, float * dis);
/* Same with a row filter (LSB-first bitmap over the ny base rows, 1 = candidate): lets the host's searchWrapper
 * (src/VectorIndex/Storages/MergeTreeVSManager.cpp:1612-1633) drop lightweight-deleted rows inside the scan instead of
 * over-fetching k + delete_id_num and filtering afterwards -- the two are equivalent (top-k of the alive rows). */
MSVS_API int msvs_knn_f32_filtered(const float * x, const float * y, size_t d, size_t k, size_t nx, size_t ny,
                                   int metric, const uint64_t * alive_bits, int64_t * ids, float * dis);

/* VectorDataset<FloatVector>::normalize() (src/VectorIndex/Common/VectorDataset.h:98-117) on the device:
 * sequential f32 sum of squares, rows with sum < FLT_EPSILON untouched, x /= sqrt(sum). In place, HOST pointer. */
MSVS_API int msvs_normalize_f32(float * x, size_t n, size_t d);
/* Binary vectors (FixedString(N) columns, nbytes = N = dimension / 8): replaces
 *   faiss::hammings_knn_mc(x, y, nx, ny, k, d / 8, (int32_t *)distance, result_id, nullptr)
 *   jaccard_knn(x, y, nx, ny, k, d / 8, distance, result_id, nullptr)
 * behind tryBruteForceSearch<BinaryVector> (src/VectorIndex/Common/BruteForceSearch.h:94-110).
 * metric: MSVS_METRIC_HAMMING (popcount(x ^ y), reported as a float like the reference's Float32 distance column) or
 * MSVS_METRIC_JACCARD ((|x | y| - |x & y|) / |x | y|, 1 for two zero vectors); anything else -> MSVS_ERR_NOT_IMPLEMENTED.
 * alive_bits: nullable LSB-first bitmap over the ny rows.  Results ascending by (distance, row), unfilled slots id -1
 * with distance FLT_MAX.  k <= MSVS_MAX_K. */
MSVS_API int msvs_knn_bin(const uint8_t * x, const uint8_t * y, size_t nbytes, size_t k, size_t nx, size_t ny,
                          int metric, const uint64_t * alive_bits, int64_t * ids, float * dis);
/* The same search and the same definition of its result with k <= MSVS_MAX_K_ROUNDS (MSVS_ERR_UNSUPPORTED_K beyond); for
 * k <= MSVS_MAX_K the same bits.  Beyond MSVS_MAX_K the scan runs once per MSVS_MAX_K ranks for the whole batch, each time behind
 * the last (distance, row) the query has returned -- see msvs_bin_index_search_rounds.  msvs_knn_bin keeps refusing k > MSVS_MAX_K. */
MSVS_API int msvs_knn_bin_rounds(const uint8_t * x, const uint8_t * y, size_t nbytes, size_t k, size_t nx, size_t ny,
                                 int metric, const uint64_t * alive_bits, int64_t * ids, float * dis);

/* Seam A1 for BinaryVector -- Search::VectorIndex<IS, OS, Bitmap, DataType::BinaryVector> (VICommon.h:142-143; the host creates
 * it at VIWithDataPart.cpp:431-446 and searches it at :928-935; index types BinaryFLAT / BinaryMSTG, goldens 00038): an
 * exhaustive Hamming / Jaccard scan (msvs_knn_bin's arithmetic) over rows kept RESIDENT on the device.  rows: n * nbytes
 * (a FixedString(N) column, 8 bits per byte); ids: the rows' labels (part row offsets; NULL = staging order); alive_bits:
 * nullable LSB-first bitmap over LABELS (nbits of them).  Files "data_bin" / "id_list" through the caller's stream openers like
 * the float index.  Results ascending by (distance, label), unfilled slots id -1 / FLT_MAX. */
typedef struct msvs_bin_index msvs_bin_index_t;
MSVS_API int msvs_bin_index_create(size_t nbytes, int metric, msvs_bin_index_t ** out);
MSVS_API void msvs_bin_index_free(msvs_bin_index_t * index);
MSVS_API int msvs_bin_index_add(msvs_bin_index_t * index, const uint8_t * rows, const int64_t * ids, size_t n);
MSVS_API size_t msvs_bin_index_num_data(const msvs_bin_index_t * index);
MSVS_API int msvs_bin_index_search(const msvs_bin_index_t * index, const uint8_t * x, size_t nx, size_t k, const uint64_t * alive_bits,
                                   size_t nbits, int64_t * ids, float * dis);
struct msvs_io;
MSVS_API int msvs_bin_index_serialize_io(const msvs_bin_index_t * index, const struct msvs_io * io);
MSVS_API int msvs_bin_index_load_io(const struct msvs_io * io, msvs_bin_index_t ** out);

/* The PARTITIONED form of the binary index (the partition scan of BinaryMSTG): ncentroids bit vectors (k-majority centroids) and
 * the rows grouped by list, searched by probing the nprobe nearest lists.  Integer popcounts throughout:
 *   - the coarse distance is Hamming for both index metrics; a row belongs to the list with the smallest (distance, list id);
 *     inside a list the rows are in ascending label order;
 *   - a query probes the first min(nprobe, ncentroids) lists by (Hamming distance to the centroid, list id); the result is the
 *     first k alive rows of those lists by (metric distance, label), unfilled slots id -1 / FLT_MAX;  k <= MSVS_MAX_K.
 * create_ivf: params "ncentroids=N[,niter=I]" (defaults 1024, 10; parsed like msvs_index_create's).  The index is NOT READY
 * (add and search return MSVS_ERR_NOT_READY) until it has centroids from train, set_centroids or a loaded file.
 * train: seeds = ncentroids rows at evenly spaced positions (no RNG), then niter rounds of exact assignment + per-bit majority vote
 * (a bit is set iff 2 * ones > members; an empty list keeps its centroid); deterministic; n < ncentroids -> MSVS_ERR_INVALID_ARGUMENT.
 * set_centroids: nlist must equal ncentroids.  num_lists: 0 for a flat index.
 * search_params: params "nprobe=P" (NULL / "": 1, the float IVFFLAT default); msvs_bin_index_search on a partitioned index is
 * search_params with the default; on a flat index nprobe is ignored.
 * export: list-major (centroids ncentroids * nbytes, ncentroids + 1 offsets, rows, labels) like msvs_index_export; NULL outputs
 * are skipped.
 * Files: a flat index writes version 1 exactly as before; a partitioned one writes version 2 (ncentroids in the header's reserved
 * words, the centroids after the rows); rows and labels stay in insertion order, the lists are rebuilt from the centroids. */
MSVS_API int msvs_bin_index_create_ivf(size_t nbytes, int metric, const char * params, msvs_bin_index_t ** out);
MSVS_API int msvs_bin_index_train(msvs_bin_index_t * index, const uint8_t * rows, size_t n);
MSVS_API int msvs_bin_index_set_centroids(msvs_bin_index_t * index, const uint8_t * centroids, size_t nlist);
MSVS_API size_t msvs_bin_index_num_lists(const msvs_bin_index_t * index);
MSVS_API int msvs_bin_index_search_params(const msvs_bin_index_t * index, const uint8_t * x, size_t nx, size_t k, const char * params,
                                          const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_bin_index_export(const msvs_bin_index_t * index, uint8_t * centroids, int64_t * list_off, uint8_t * rows,
                                   int64_t * labels);
/* k beyond MSVS_MAX_K, and device pointers, for both forms of the binary index.  The result is defined exactly as above: the first k
 * alive rows (of the probed lists) by (distance, label), unfilled slots -1 / FLT_MAX.
 * search_rounds (host pointers): k <= MSVS_MAX_K_ROUNDS (MSVS_ERR_UNSUPPORTED_K beyond); params NULL, "" or "nprobe=P" as
 *   search_params; for k <= MSVS_MAX_K the same bits as search / search_params.  Beyond MSVS_MAX_K the scan runs once per MSVS_MAX_K
 *   ranks for the whole batch, each time behind the last (distance, label) the query has returned.  Hamming distances are small
 *   integers, so such a boundary usually lies inside a run of equal distances: the label decides there, exactly.  Two rows that carry
 *   the SAME label at the same distance are returned once when they straddle such a boundary (labels are expected to be distinct).
 * search_device: d_x (nx dense rows of nbytes), d_alive_bits (nullable, ceil(nbits / 64) words), d_ids and d_dis ([nx][k]) are DEVICE
 *   pointers; everything is enqueued on hip_stream and nothing waits for the host -- except at the first search (on this device)
 *   after an add, train or set_centroids, which builds the index's device image and synchronises hip_stream while it does.  The index
 *   must not be added to or freed before hip_stream has run the search.  k <= MSVS_MAX_K; nprobe as search_params' (a flat index
 *   ignores it, a partitioned one wants nprobe >= 1: MSVS_ERR_INVALID_ARGUMENT); a null buffer with nx > 0 and k > 0 is
 *   MSVS_ERR_INVALID_ARGUMENT; k = 0 or nx = 0 is a no-op; a partitioned index without centroids is MSVS_ERR_NOT_READY.  The same
 *   bits as search_params.
 * search_rounds_device: search_device with k <= MSVS_MAX_K_ROUNDS, the rounds run back to back on hip_stream.
 * search, search_params and search_device keep refusing k > MSVS_MAX_K. */
MSVS_API int msvs_bin_index_search_rounds(const msvs_bin_index_t * index, const uint8_t * x, size_t nx, size_t k, const char * params,
                                          const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_bin_index_search_device(const msvs_bin_index_t * index, const uint8_t * d_x, size_t nx, size_t k, size_t nprobe,
                                          const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream);
MSVS_API int msvs_bin_index_search_rounds_device(const msvs_bin_index_t * index, const uint8_t * d_x, size_t nx, size_t k, size_t nprobe,
                                                 const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                 void * hip_stream);

/* IVFSQ -- an inverted-file index of Float32 vectors that keeps 8-bit residual codes ONLY (no f32 row survives build): dim bytes
 * (padded to 16) + a u32 label per row; 4-bit codes or binary16 residuals with bit_size=4 / 16 (below).  metric: L2 / IP / COSINE (anything else -> MSVS_ERR_NOT_IMPLEMENTED).  All arithmetic
 * is f32 with separately rounded operations (fl), no fma, IEEE division:
 *   - contents: nlist centroids c_l; ONE quantiser vmin[j], vmax[j] per dimension, step[j] = fl(fl(vmax[j] - vmin[j]) / 255);
 *     per row its list, label and dim codes; rows inside a list in ascending label order;
 *   - stored row x: the row as fed (L2, IP) or the normalised row (cosine; msvs_normalize_f32's arithmetic);
 *   - encode in list l: r = fl(x_j - c_lj), t = fl(fl(r - vmin[j]) / step[j]), code = min(255, max(0, rint(t))) (ties to even),
 *     0 where step[j] == 0; rows outside the trained range are clamped;
 *     a NaN residual (a NaN in the row, or inf - inf) has code 0, +inf the top code and -inf code 0, at 8 and at 4 bits;
 *   - decode: x^_j = fl(c_lj + fl(vmin[j] + fl(float(code) * step[j])));
 *   - search = the IVFFLAT search of the decoded rows: the canonical exact top-min(nprobe, nlist) lists by (distance to the
 *     centroid, list id), every alive row of them scored with the canonical scan arithmetic over x^, top-k by (distance, label),
 *     unfilled slots -1 and the metric's neutral value; cosine normalises the query, searches with IP and reports fl(1 - ip) in
 *     every slot; the filter is indexed by label.  The search over what the index stores is exact; the quantiser is lossy.
 *   - a row is assigned to its nearest centroid by L2 (L2 indexes) or by inner product (IP and cosine), as msvs_index_add does.
 *     Its rule for a row without a finite score: the score of centroid l is |c_l|^2 - 2 <c_l, x> (L2) or -<c_l, x>; the smallest
 *     score that is not NaN and not above FLT_MAX wins, -inf included, the lowest l among equals; a row all of whose scores are NaN
 *     or +inf goes to list 0.
 *   - bit_size=4 (create): the same index with 4-bit codes, two a stored byte: step[j] = fl(fl(vmax[j] - vmin[j]) / 15),
 *     code = min(15, max(0, rint(t))) (ties to even), 0 where step[j] == 0; t, decode, training, the trained range, set_codebook's
 *     checks and the clamping of rows outside the range as above.
 *   - bit_size=16 (create): the code is the IEEE binary16 value nearest to r = fl(x_j - c_lj), round to nearest even, binary16
 *     subnormals kept in both directions, overflow to +-inf, a NaN stays a NaN; decode: x^_j = fl(c_lj + float(h)), the conversion
 *     to f32 being exact.  vmin / vmax keep their place in train, set_codebook, export and the file -- computed, validated, stored
 *     and returned exactly as at 8 bits, so that there is one file layout and one binding -- but NEITHER enters encode or decode:
 *     no row is clamped.  They remain the exact range of the training residuals, from which a host can see that nothing
 *     approaches 65504.
 *   Everything else -- the definition of search, assignment, labels, the filter, cosine, the limits of k and nprobe, search_rounds,
 *   search_refine[_rounds] and their device forms -- is shared by the three widths.
 * create: params as msvs_index_create's for IVFFLAT (ncentroids, kmeans_iters, train_sample, seed, ...) and bit_size, the bits of a
 *   code: 8 (the default), 4 or 16, anything else MSVS_ERR_INVALID_ARGUMENT; without bit_size, or with bit_size=8, every result,
 *   every file byte and every error code is what it was.  dim is bounded by the scan's LDS stage (round_up(dim, 16) <= 2240) at
 *   every width, checked here and at load.
 * train: the IVFFLAT k-means over the rows, then vmin / vmax = exact minimum / maximum of the residuals of ALL n training rows
 *   against their assigned centroids; the same input gives the same bits.  set_codebook: centroids and quantiser from the caller.
 *   (vmin / vmax must be finite with vmax >= vmin: MSVS_ERR_INVALID_ARGUMENT otherwise).  At 8 and 4 bits fl(vmax[j] - vmin[j]) must
 *   be finite too, or the step is infinite and every row decodes to NaN: set_codebook refuses such bounds and train refuses rows whose
 *   residuals span such a range (one infinite element is enough), both with MSVS_ERR_INVALID_ARGUMENT and without leaving a codebook;
 *   load refuses such a file with MSVS_ERR_IO.  At bit_size=16 train accepts them: the range enters no arithmetic.  Both must precede add
 *   (MSVS_ERR_NOT_READY from add before either).
 * add: any number of chunks before build; rows are encoded as they arrive, only codes, lists and labels are staged.  ids: labels
 *   in [0, 2^32 - 1) (MSVS_ERR_ID_RANGE otherwise), NULL = staging order; labels are expected to be distinct, as for
 *   msvs_index_add (a repeated label is not rejected).
 * search (host pointers): params "nprobe=P" (default 1).  search_device: device pointers, enqueued on hip_stream without host
 *   synchronisation.  k <= MSVS_MAX_K and min(nprobe, nlist) <= MSVS_MAX_K (MSVS_ERR_UNSUPPORTED_K); k = 0 or nq = 0 is a no-op;
 *   before build: MSVS_ERR_NOT_READY.
 * search_rounds / search_rounds_device: the same search and the same definition of its result with k <= MSVS_MAX_K_ROUNDS
 *   (MSVS_ERR_UNSUPPORTED_K beyond); everything else as search / search_device, and for k <= MSVS_MAX_K the same bits.  Beyond
 *   MSVS_MAX_K the list scan runs once per MSVS_MAX_K ranks for the whole batch, each time behind the last (distance, label) the
 *   query has returned: two rows that carry the SAME label at the same distance are returned once when they straddle such a
 *   boundary (labels are expected to be distinct).  search / search_device keep refusing k > MSVS_MAX_K.
 * search_rounds / search_rounds_device: the same search and the same definition of its result with k <= MSVS_MAX_K_ROUNDS
 *   (MSVS_ERR_UNSUPPORTED_K beyond); everything else as search / search_device, and for k <= MSVS_MAX_K the same bits.  Beyond
 *   MSVS_MAX_K the list scan runs once per MSVS_MAX_K ranks for the whole batch, each time behind the last (distance, label) the
 *   query has returned: two rows that carry the SAME label at the same distance are returned once when they straddle such a
 *   boundary (labels are expected to be distinct).  search / search_device keep refusing k > MSVS_MAX_K.
 * export: centroids nlist * dim, vmin / vmax dim each, nlist + 1 offsets, codes n * dim in NATURAL column order, labels n; any
 *   output may be NULL.  bit_size=4: one code a byte (values < 16), n * dim bytes.  bit_size=16: `codes` receives n * dim
 *   little-endian uint16 bit patterns, 2 * n * dim bytes.  bit_size: 4, 8 or 16 (0 for NULL): what a host that loaded an index
 *   sizes export's buffer by.
 * memory_usage after build <= n * (round_up(dim, 16) + 8) + the centroids, quantiser and offsets + 4096 bytes; the row term is
 *   round_up(ceil(dim / 2), 16) + 8 at bit_size=4 and 2 * round_up(dim, 16) + 8 at bit_size=16.
 * Files "sq_data" / "sq_ids" through the caller's stream openers (a built index only); load validates sizes, offsets, labels and
 * a checksum of each header: a corrupt or truncated file is MSVS_ERR_IO.  The data file's 56-byte header carries the code width
 * in its `reserved` word: 0 for 8 bits (the files of before bit_size, byte for byte), 4 or 16; any other value is MSVS_ERR_IO.
 * Its codes section is n * dim bytes (8), n * ceil(dim / 2) bytes with code j in the low (even j) or high nibble of byte j / 2 and a
 * zero pad nibble at odd dim (4; a non-zero one is MSVS_ERR_IO), or 2 * n * dim bytes, little endian (16), in natural order. */
typedef struct msvs_sq_index msvs_sq_index_t;
MSVS_API int msvs_sq_index_create(int metric, size_t dim, const char * params, msvs_sq_index_t ** out);
MSVS_API void msvs_sq_index_free(msvs_sq_index_t * index);
MSVS_API int msvs_sq_index_train(msvs_sq_index_t * index, const float * x, size_t n, int mem);
MSVS_API int msvs_sq_index_set_codebook(msvs_sq_index_t * index, const float * centroids, size_t nlist, const float * vmin,
                                        const float * vmax, int mem);
MSVS_API int msvs_sq_index_add(msvs_sq_index_t * index, const float * x, const int64_t * ids, size_t n, int mem);
MSVS_API int msvs_sq_index_build(msvs_sq_index_t * index);
MSVS_API int msvs_sq_index_ready(const msvs_sq_index_t * index);
MSVS_API size_t msvs_sq_index_num_data(const msvs_sq_index_t * index);
MSVS_API size_t msvs_sq_index_num_lists(const msvs_sq_index_t * index);
MSVS_API size_t msvs_sq_index_memory_usage(const msvs_sq_index_t * index);
MSVS_API size_t msvs_sq_index_bit_size(const msvs_sq_index_t * index);
MSVS_API int msvs_sq_index_search(const msvs_sq_index_t * index, const float * queries, size_t nq, size_t k, const char * params,
                                  const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_sq_index_search_device(const msvs_sq_index_t * index, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                         const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                         void * hip_stream);
MSVS_API int msvs_sq_index_search_rounds(const msvs_sq_index_t * index, const float * queries, size_t nq, size_t k, const char * params,
                                         const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_sq_index_search_rounds_device(const msvs_sq_index_t * index, const float * d_queries, size_t nq, size_t k,
                                                size_t nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                                float * d_dis, void * hip_stream);
MSVS_API int msvs_sq_index_export(const msvs_sq_index_t * index, float * centroids, float * vmin, float * vmax, int64_t * list_off,
                                  uint8_t * codes, int64_t * ids);
MSVS_API int msvs_sq_index_serialize_io(const msvs_sq_index_t * index, const struct msvs_io * io);
MSVS_API int msvs_sq_index_load_io(const struct msvs_io * io, msvs_sq_index_t ** out);

/* IVFPQ -- an inverted-file index of Float32 vectors that keeps product-quantised residual codes ONLY (no f32 row survives build):
 * m code bytes, or ceil(m / 2) at bit_size=4, (padded to 4) + a u32 label per row.  metric: L2 / IP / COSINE (anything else -> MSVS_ERR_NOT_IMPLEMENTED).  All
 * arithmetic is f32 with separately rounded operations (fl), no fma:
 *   - contents: nlist centroids c_l; m sub-codebooks cb[s][j] (s < m, j < ksub = 1 << bit_size: 256 entries, or 16 at bit_size=4) of
 *     dsub = dim / m floats each; per row its list, label and m codes; rows inside a list in ascending label order;
 *   - stored row x: the row as fed (L2, IP) or the normalised row (cosine; msvs_normalize_f32's arithmetic);
 *   - decoded sub-vector of code j in sub-space s of list l: x^[t] = fl(c_l[s * dsub + t] + cb[s][j][t]), t < dsub;
 *   - sub-score e of a (query or row) sub-vector q against x^, t ascending, a sequential sum starting at +0:
 *     L2: sum of fl(fl(q_t - x^_t)^2); IP and cosine: sum of fl(q_t * x^_t);
 *   - encode (every metric): code[s] = the j with the smallest L2 sub-score between the stored row's sub-vector and x^; ties go to the
 *     lowest j; a NaN score never wins (all NaN: code 0);
 *   - distance of a row: dis = +0, then dis = fl(dis + e(s, code[s])) for s = 0 .. m - 1 (the ADC sum over a per-(query, list)
 *     look-up table); it equals a distance to the decoded row with the sums taken per sub-space first;
 *   - search: the canonical exact top-min(nprobe, nlist) lists by (distance to the centroid, list id), every alive row of them
 *     scored as above, top-k by (distance asc -- desc for IP --, label asc), strictly better than the metric's neutral value
 *     (+-FLT_MAX), unfilled slots -1 and that value; cosine normalises the query, searches with IP and reports fl(1 - ip) in every
 *     slot; the filter is indexed by label.  The search over what the index stores is exact; the quantiser is lossy.
 *   - a row is assigned to its nearest centroid by L2 (L2 indexes) or by inner product (IP and cosine), as msvs_index_add does.
 *     Its rule for a row without a finite score: the score of centroid l is |c_l|^2 - 2 <c_l, x> (L2) or -<c_l, x>; the smallest
 *     score that is not NaN and not above FLT_MAX wins, -inf included, the lowest l among equals; a row all of whose scores are NaN
 *     or +inf goes to list 0.
 * create: params as msvs_index_create's for IVFFLAT (ncentroids, kmeans_iters, train_sample, seed, ...) plus m, the number of
 *   sub-quantisers (required), and bit_size, the bits of a code: 8 (the default) or 4, anything else MSVS_ERR_INVALID_ARGUMENT.
 *   bit_size=8: 1 <= m <= 128, m divides dim, dim <= 8192, and the list scan's smallest LDS image, m KiB of tables +
 *   8 * round_up(dim, 4) + 5 * 8 * MSVS_MAX_K bytes, fits 160 KiB.  bit_size=4: 1 <= m <= 256, m divides dim, dim <= 8192 (the image,
 *   64 * m + 8 * round_up(dim, 4) + 5 * 8 * MSVS_MAX_K bytes, always fits); a row keeps ceil(m / 2) code bytes (padded to 4, pad
 *   nibbles 0).  MSVS_ERR_INVALID_ARGUMENT otherwise, checked here and at load.  With ksub in place of 256 everything above and
 *   below holds for both; without bit_size, or with bit_size=8, every result and every file byte is what it was.
 * train: the coarse centroids by the IVFFLAT k-means over the rows; then the residuals fl(x - c_l) of at most 262144 training rows
 *   (row floor(i * n / cap), i < cap = min(n, 262144)); for every s the dsub columns of sub-space s go through the same k-means
 *   (L2, ksub centroids, the same iterations and seed): its centroids are cb[s].  n < ksub: MSVS_ERR_INVALID_ARGUMENT.  The same input
 *   gives the same bits.  Training rows with NaN or infinite elements: a coarse centroid or a codebook entry that comes out non-finite
 *   is MSVS_ERR_INVALID_ARGUMENT and leaves the index without a codebook, as set_codebook does (such a row that no trainer's sample
 *   holds changes nothing): train never leaves a non-finite codebook.  set_codebook: centroids (nlist * dim) and codebooks (m * ksub * dsub, [s][j][t]) from the caller; a
 *   non-finite codebook entry is MSVS_ERR_INVALID_ARGUMENT and leaves the index without a codebook.  Both must precede add
 *   (MSVS_ERR_NOT_READY from add before either; MSVS_ERR_INVALID_ARGUMENT from either after add).
 * add: any number of chunks before build; rows are encoded as they arrive, only codes, lists and labels are staged.  ids: labels
 *   in [0, 2^32 - 1) (MSVS_ERR_ID_RANGE otherwise), NULL = staging order; labels are expected to be distinct.
 * search (host pointers): params "nprobe=P" (default 1).  search_device: device pointers, enqueued on hip_stream without host
 *   synchronisation.  k <= MSVS_MAX_K and min(nprobe, nlist) <= MSVS_MAX_K (MSVS_ERR_UNSUPPORTED_K); k = 0 or nq = 0 is a no-op;
 *   before build: MSVS_ERR_NOT_READY.
 * search_rounds / search_rounds_device: the same search and the same definition of its result with k <= MSVS_MAX_K_ROUNDS
 *   (MSVS_ERR_UNSUPPORTED_K beyond); everything else as search / search_device, and for k <= MSVS_MAX_K the same bits.  Beyond
 *   MSVS_MAX_K the list scan runs once per MSVS_MAX_K ranks for the whole batch, each time behind the last (distance, label) the
 *   query has returned: two rows that carry the SAME label at the same distance are returned once when they straddle such a
 *   boundary (labels are expected to be distinct).  search / search_device keep refusing k > MSVS_MAX_K.
 * search_rounds / search_rounds_device: the same search and the same definition of its result with k <= MSVS_MAX_K_ROUNDS
 *   (MSVS_ERR_UNSUPPORTED_K beyond); everything else as search / search_device, and for k <= MSVS_MAX_K the same bits.  Beyond
 *   MSVS_MAX_K the list scan runs once per MSVS_MAX_K ranks for the whole batch, each time behind the last (distance, label) the
 *   query has returned: two rows that carry the SAME label at the same distance are returned once when they straddle such a
 *   boundary (labels are expected to be distinct).  search / search_device keep refusing k > MSVS_MAX_K.
 * export: centroids nlist * dim, codebooks m * ksub * dsub, nlist + 1 offsets, codes n * m in NATURAL order, one code a byte in both
 *   forms (values < ksub), labels n; any output may be NULL.  bit_size: 4 or 8 (0 for NULL): what a host that loaded an index
 *   sizes export's codebook buffer by.
 * memory_usage after build <= n * (round_up(m, 16) + 8) + the centroids, codebooks and offsets + 4096 bytes; at bit_size=4
 *   <= n * (round_up(ceil(m / 2), 16) + 8) + the centroids, 16 * dim * 4 bytes of codebooks, the offsets + 4096 bytes.
 * Files "pq_data" (header "MSVSPQ01", centroids, codebooks, offsets, codes in natural order) / "pq_ids" through the caller's stream
 * openers (a built index only); load validates sizes, offsets, labels, the codebooks and a checksum of each header: a corrupt or
 * truncated file is MSVS_ERR_IO.  The header's reserved word is 0 for an 8-bit index and 4 for a 4-bit one, whose codes are
 * n * ceil(m / 2) bytes, code s in the low nibble of byte s / 2 for even s, else the high one; any other reserved word, an m beyond
 * the form's limit and a non-zero pad nibble (odd m) are MSVS_ERR_IO too (a library without the 4-bit form refuses such a file).
 *
 * query_tables=1 (create; 0 is the default, anything else MSVS_ERR_INVALID_ARGUMENT; both bit sizes, all three metrics): look-up tables
 * that depend on the query alone.  Codebooks, training, assignment and the codes are exactly what they are without it -- a row's
 * codes are the same bytes in both forms; only the distance of a row is another sum, and an L2 index keeps one f32 more per row.
 * With q the query (normalised first for cosine), c = c_l, fl as above, no fma:
 *   - query table (no list in it): P[s][j] = the sequential sum from +0, t ascending, of fl(q[s * dsub + t] * cb[s][j][t]);
 *   - row term (L2 indexes only, per stored row of list l): g(s) = the sequential sum from +0, t ascending, of
 *     fl(cb_t * fl(fl(c_t + c_t) + cb_t)) with cb = cb[s][code[s]] and c_t = c_l[s * dsub + t]; w = +0, then w = fl(w + g(s)) for
 *     s = 0 .. m - 1.  The library computes w at build and at load; no file holds it;
 *   - pair term: b(q, l) = the canonical distance (L2) or inner product (IP, cosine) of q to c_l, the value the lists are ranked by;
 *   - row score: acc = +0, then acc = fl(acc + P[s][code[s]]), s ascending; L2: dis = fl(fl(b + w) - fl(2 * acc)); IP and cosine:
 *     dis = fl(b + acc).
 * Admission, order, padding, cosine's fl(1 - ip), the filter, the probes and the limits on k and nprobe are those above.  It equals
 * |q - (c + cb)|^2 (q . (c + cb)) up to rounding, with another summation order than the default form: results of the two forms differ
 * in their last bits.  query_tables: 1 for such an index, else 0 (0 for NULL).  export_row_terms: w of the n rows in list-major order
 * (export's); MSVS_ERR_INVALID_ARGUMENT for an index that keeps none (query_tables=0, IP, cosine), MSVS_ERR_NOT_READY before build.
 * memory_usage: the bound above + 4 * n for an L2 index of this form only.  Files: bit 8 of the header's reserved word is set (0x100
 * for 8-bit codes, 0x104 for 4-bit), every other byte of pq_data but the check word, and all of pq_ids, is the file of the same index
 * without the form; every other reserved word stays MSVS_ERR_IO (a library without the form refuses such a file).  Without
 * query_tables, or with query_tables=0, every result, every file byte and every error is what it was. */
typedef struct msvs_pq_index msvs_pq_index_t;
MSVS_API int msvs_pq_index_create(int metric, size_t dim, const char * params, msvs_pq_index_t ** out);
MSVS_API void msvs_pq_index_free(msvs_pq_index_t * index);
MSVS_API int msvs_pq_index_train(msvs_pq_index_t * index, const float * x, size_t n, int mem);
MSVS_API int msvs_pq_index_set_codebook(msvs_pq_index_t * index, const float * centroids, size_t nlist, const float * codebooks,
                                        int mem);
MSVS_API int msvs_pq_index_add(msvs_pq_index_t * index, const float * x, const int64_t * ids, size_t n, int mem);
MSVS_API int msvs_pq_index_build(msvs_pq_index_t * index);
MSVS_API int msvs_pq_index_ready(const msvs_pq_index_t * index);
MSVS_API size_t msvs_pq_index_num_data(const msvs_pq_index_t * index);
MSVS_API size_t msvs_pq_index_num_lists(const msvs_pq_index_t * index);
MSVS_API size_t msvs_pq_index_memory_usage(const msvs_pq_index_t * index);
MSVS_API size_t msvs_pq_index_bit_size(const msvs_pq_index_t * index);
MSVS_API int msvs_pq_index_query_tables(const msvs_pq_index_t * index);
MSVS_API int msvs_pq_index_export_row_terms(const msvs_pq_index_t * index, float * w);
MSVS_API int msvs_pq_index_search(const msvs_pq_index_t * index, const float * queries, size_t nq, size_t k, const char * params,
                                  const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_pq_index_search_device(const msvs_pq_index_t * index, const float * d_queries, size_t nq, size_t k, size_t nprobe,
                                         const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                         void * hip_stream);
MSVS_API int msvs_pq_index_search_rounds(const msvs_pq_index_t * index, const float * queries, size_t nq, size_t k, const char * params,
                                         const uint64_t * alive_bits, size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_pq_index_search_rounds_device(const msvs_pq_index_t * index, const float * d_queries, size_t nq, size_t k,
                                                size_t nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                                float * d_dis, void * hip_stream);
MSVS_API int msvs_pq_index_export(const msvs_pq_index_t * index, float * centroids, float * codebooks, int64_t * list_off,
                                  uint8_t * codes, int64_t * ids);
MSVS_API int msvs_pq_index_serialize_io(const msvs_pq_index_t * index, const struct msvs_io * io);
MSVS_API int msvs_pq_index_load_io(const struct msvs_io * io, msvs_pq_index_t ** out);

/* Two-stage search -- the exact re-rank of a coded index's candidates (Faiss: IndexRefineFlat; the reference's index interface:
 * computeTopDistanceSubset / supportTwoStageSearch).  IVFSQ and IVFPQ return labels with the quantiser's distances; scored again
 * against the original f32 rows, the best k of kc candidates carry the canonical distances FLAT and IVFFLAT report.
 *
 * Row store (msvs_rows_*): an append-only table of f32 rows in which ROW i IS LABEL i -- part-local row offsets, the labels the coded
 * indexes carry when add gets ids = NULL.  Row stride round_up(dim, 4) floats, zero padded.
 *   create: 1 <= dim <= 8192 and placement MSVS_ROWS_DEVICE / MSVS_ROWS_HOST_PINNED (MSVS_ERR_INVALID_ARGUMENT otherwise);
 *     capacity_rows is fixed here and <= 2^32 - 1 (MSVS_ERR_ID_RANGE otherwise).  normalize != 0 stores msvs_normalize_f32's rows
 *     (the same arithmetic, the same skip of rows whose norm is below FLT_EPSILON), as msvs_block_upload does for cosine.
 *     MSVS_ROWS_HOST_PINNED keeps the table in mapped, pinned host memory, which the kernel reads directly: only labels and queries
 *     live in device memory, and the kernel is the same for both placements.
 *   append: chunks of n dense rows, host or device (mem), like the indexes' add; beyond the capacity: MSVS_ERR_INVALID_ARGUMENT (and
 *     nothing is appended).  Not concurrent with a refine; refines are re-entrant on a store that is no longer appended to.
 *   num / dim / normalized: what the store holds (0 for NULL).  memory_usage: DEVICE bytes -- the table for MSVS_ROWS_DEVICE, 0 for
 *     a pinned store.  There are no files: the rows are the part's column, the host feeds them again.
 *
 * refine (host pointers; stages, runs, copies back, synchronises) / refine_device (device pointers, enqueued on hip_stream without
 * host synchronisation): queries nq * dim, cand nq * kc labels, ids / dis nq * k.  For each query:
 *   - every candidate label c with 0 <= c < msvs_rows_num is scored against stored row c with the canonical scan arithmetic: 64
 *     partial sums (accumulator e mod 64 for element e), multiply and add separately rounded, no fma, folded by the adjacent pairwise
 *     tree -- the arithmetic of msvs_knn_f32 and the FLAT / IVFFLAT searches, bit for bit;
 *   - labels < 0 (the first stage's padding) are skipped wherever they stand in the list, labels >= num too;
 *   - a label that occurs twice is returned as often as it occurs;
 *   - a candidate enters only if strictly better than the metric's neutral value (+-FLT_MAX); NaN never enters;
 *   - order: (distance ascending -- descending for IP --, then label ascending); unfilled slots are -1 and the neutral value;
 *   - cosine needs a store created with normalize=1, L2 and IP one with normalize=0 (MSVS_ERR_INVALID_ARGUMENT otherwise); cosine
 *     normalises the queries, searches with IP and reports fl(1 - ip) in every slot, as the indexes do;
 *   - k <= MSVS_MAX_K and kc <= MSVS_REFINE_MAX_CAND (MSVS_ERR_UNSUPPORTED_K beyond either); k may exceed kc, the rest are pads;
 *     k = 0 or nq = 0 is a no-op; a metric outside L2 / IP / COSINE -> MSVS_ERR_NOT_IMPLEMENTED; null arguments ->
 *     MSVS_ERR_INVALID_ARGUMENT.
 *
 * search_refine[_device] of the coded indexes: the index's own search[_device] with kc results (kc <= MSVS_MAX_K; params / nprobe
 * and the filter apply here), the labels kept on the device, then refine_device with the index's metric -- no host round trip between
 * the stages.  rows' dim must be the index's and normalized == (metric is cosine), and k <= kc: MSVS_ERR_INVALID_ARGUMENT otherwise.
 * The result equals refine applied to search(kc)'s labels.
 * search_refine_rounds[_device]: the same with search_rounds[_device] as the first stage: kc <= MSVS_REFINE_MAX_CAND and
 * k <= MSVS_MAX_K (MSVS_ERR_UNSUPPORTED_K beyond either), k <= kc and the row store's fit as above; the result equals refine applied
 * to search_rounds(kc)'s labels, and for kc <= MSVS_MAX_K search_refine's.  search_refine[_device] keep refusing kc > MSVS_MAX_K. */
#define MSVS_REFINE_MAX_CAND 1024
typedef struct msvs_rows msvs_rows_t;
enum msvs_rows_placement { MSVS_ROWS_DEVICE = 0, MSVS_ROWS_HOST_PINNED = 1 };
MSVS_API int msvs_rows_create(size_t dim, int normalize, int placement, size_t capacity_rows, msvs_rows_t ** out);
MSVS_API int msvs_rows_append(msvs_rows_t * rows, const float * x, size_t n, int mem);
MSVS_API size_t msvs_rows_num(const msvs_rows_t * rows);
MSVS_API size_t msvs_rows_dim(const msvs_rows_t * rows);
MSVS_API int msvs_rows_normalized(const msvs_rows_t * rows);
MSVS_API size_t msvs_rows_memory_usage(const msvs_rows_t * rows);
MSVS_API void msvs_rows_free(msvs_rows_t * rows);
MSVS_API int msvs_refine(const msvs_rows_t * rows, int metric, const float * queries, size_t nq, const int64_t * cand, size_t kc,
                         size_t k, int64_t * ids, float * dis);
MSVS_API int msvs_refine_device(const msvs_rows_t * rows, int metric, const float * d_queries, size_t nq, const int64_t * d_cand,
                                size_t kc, size_t k, int64_t * d_ids, float * d_dis, void * hip_stream);
MSVS_API int msvs_sq_index_search_refine(const msvs_sq_index_t * index, const msvs_rows_t * rows, const float * queries, size_t nq,
                                         size_t k, size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits,
                                         int64_t * ids, float * dis);
MSVS_API int msvs_sq_index_search_refine_device(const msvs_sq_index_t * index, const msvs_rows_t * rows, const float * d_queries,
                                                size_t nq, size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits,
                                                size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream);
MSVS_API int msvs_sq_index_search_refine_rounds(const msvs_sq_index_t * index, const msvs_rows_t * rows, const float * queries,
                                                size_t nq, size_t k, size_t kc, const char * params, const uint64_t * alive_bits,
                                                size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_sq_index_search_refine_rounds_device(const msvs_sq_index_t * index, const msvs_rows_t * rows,
                                                       const float * d_queries, size_t nq, size_t k, size_t kc, size_t nprobe,
                                                       const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                       void * hip_stream);
MSVS_API int msvs_pq_index_search_refine(const msvs_pq_index_t * index, const msvs_rows_t * rows, const float * queries, size_t nq,
                                         size_t k, size_t kc, const char * params, const uint64_t * alive_bits, size_t nbits,
                                         int64_t * ids, float * dis);
MSVS_API int msvs_pq_index_search_refine_device(const msvs_pq_index_t * index, const msvs_rows_t * rows, const float * d_queries,
                                                size_t nq, size_t k, size_t kc, size_t nprobe, const uint64_t * d_alive_bits,
                                                size_t nbits, int64_t * d_ids, float * d_dis, void * hip_stream);
MSVS_API int msvs_pq_index_search_refine_rounds(const msvs_pq_index_t * index, const msvs_rows_t * rows, const float * queries,
                                                size_t nq, size_t k, size_t kc, const char * params, const uint64_t * alive_bits,
                                                size_t nbits, int64_t * ids, float * dis);
MSVS_API int msvs_pq_index_search_refine_rounds_device(const msvs_pq_index_t * index, const msvs_rows_t * rows,
                                                       const float * d_queries, size_t nq, size_t k, size_t kc, size_t nprobe,
                                                       const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids, float * d_dis,
                                                       void * hip_stream);

/* Resident blocks for the brute-force path: the GPU analogue of VICacheManager / VIWithMeta
 * (src/VectorIndex/Cache/VICacheObject.h:40-162) for the dense block a mark of a part turns into
 * (MergeTreeVSManager.cpp:1380-1392).  msvs_knn_f32 moves that block over PCIe on every query; here it is uploaded
 * once, keyed by (part key, mark) -- CacheKey::toString() is a natural part key -- and kept in HBM in an LRU bounded by
 * bytes.  Blocks are immutable: lightweight deletes arrive per search as the row_exists bitmap like in the reference
 * (searchWrapper, MergeTreeVSManager.cpp:1612-1633); a dropped / mutated part is evicted by key prefix.
 * upload: returns the resident block PINNED (an identical key already resident is returned instead -- concurrent
 * part-pool threads race benignly); normalize != 0 stores VectorDataset::normalize()'d rows (the cosine composition of
 * searchWithoutIndex normalises the block in place before the IP search).  lookup: *out = NULL when absent.
 * release unpins; a pinned block is never freed, an evicted one disappears at its last release.  Thread-safe. */
typedef struct msvs_cache msvs_cache_t;
typedef struct msvs_block msvs_block_t;
MSVS_API int msvs_cache_create(size_t capacity_bytes, msvs_cache_t ** out);
MSVS_API void msvs_cache_free(msvs_cache_t * cache);
MSVS_API int msvs_block_upload(msvs_cache_t * cache, const char * part_key, uint64_t mark, const float * rows, size_t n,
                               size_t d, int normalize, msvs_block_t ** out);
MSVS_API int msvs_block_lookup(msvs_cache_t * cache, const char * part_key, uint64_t mark, msvs_block_t ** out);
MSVS_API void msvs_block_release(msvs_block_t * block);
/* Shape and stored form of a resident block (rows, dimension, 1 = rows were normalised at upload); any out pointer may be NULL.
 * A caller that finds a block by key checks these against what it is about to search: a block uploaded for Cosine holds
 * normalised rows and must not serve an L2 / IP search of the same part (msvs_host.cpp keys the two forms apart as well). */
MSVS_API int msvs_block_info(const msvs_block_t * block, size_t * n, size_t * d, int * normalized);
MSVS_API int msvs_cache_evict(msvs_cache_t * cache, const char * key_prefix, size_t * evicted);
MSVS_API int msvs_cache_stats(msvs_cache_t * cache, size_t * bytes, size_t * blocks, uint64_t * hits, uint64_t * misses,
                              uint64_t * evictions);
/* msvs_knn_f32[_filtered] against a resident block: x nx*d (HOST), alive_bits nullable over the block's rows. */
MSVS_API int msvs_knn_resident(const msvs_block_t * block, const float * x, size_t k, size_t nx, int metric,
                               const uint64_t * alive_bits, int64_t * ids, float * dis);

/* ---------------------------------------------------------------------------------------------
 * Seam A1 -- vector index object.  Replaces Search::VectorIndex<...,FloatVector>:
 *   createVectorIndex(name, type, metric, dim, total_vec, params, ...)   VIWithDataPart.cpp:415-446
 *   build(reader, threads, cancel)  [train + chunked add]                VIWithDataPart.h:295-339, VIPartReader.h:170-304
 *   search(DataSet{nq,dim}, k, params, first_stage_only, DenseBitmap*)   VIWithDataPart.cpp:922-926
 *   ready(), numData(), getResourceUsage(), serialize()/load()           VIWithDataPart.cpp:368-385,472-479,698-700
 * The index data lives in HBM; search never touches host copies of the vectors.
 */
typedef struct msvs_index msvs_index_t;

/* params: "key=value" pairs separated by ',' or a flat JSON object, e.g. "ncentroids=1024" /
 * {"ncentroids":"1024"}.  IVFFLAT build params: ncentroids (default 1024), kmeans_iters (10),
 * train_sample (ncentroids*64), seed (1234).  Sharding for multi-GPU: shard_rank / shard_world
 * (lists with list_id % shard_world == shard_rank are kept on this device).
 * shadow (1): the second, compact copy of the rows the batched list scan streams -- 0 none, 1 auto (L2 IVFFLAT: int8
 * residuals where the rows sit close to their centroids, else fp16; every other index fp16), 2 fp16, 3 int8 residuals (L2
 * IVFFLAT only; others fp16), 4 int8 residuals whatever the metric of an IVFFLAT index (L2: the same as 3), 5 auto over
 * every metric (L2: the rule of 1; inner product and cosine: int8 residuals when every list is inside the error model's
 * range and >= 97 % of the rows sit in lists whose rounding bound is within 3x fp16's).  Results never depend on it. */
MSVS_API int msvs_index_create(int index_type, int metric, size_t dim, const char * params, msvs_index_t ** out);
MSVS_API void msvs_index_free(msvs_index_t * index);

/* IVFFLAT: k-means over the training rows (ignored by FLAT).  mem = MSVS_MEM_HOST|MSVS_MEM_DEVICE. */
MSVS_API int msvs_index_train(msvs_index_t * index, const float * x, size_t n, int mem);
/* Alternative to train: adopt given coarse centroids (nlist*dim). */
MSVS_API int msvs_index_set_centroids(msvs_index_t * index, const float * centroids, size_t nlist, int mem);
/* One chunk of the build feed: n rows (n*dim f32) + their ids (nullable => consecutive from the current count).
 * Mirrors Search::DataChunk{data, n, dim} + setDataID(ids) (VIPartReader.h:296-303). */
MSVS_API int msvs_index_add(msvs_index_t * index, const float * x, const int64_t * ids, size_t n, int mem);
/* The factory's check_cancelled callback (VIWithDataPart.cpp:425-430: BaseDaemon::isCancelled): polled between k-means
 * iterations of train, at every add and between the phases of build; nonzero -> the call returns MSVS_ERR_ABORTED
 * ("Cancelled building vector index") and the index stays unbuilt.  NULL clears it. */
MSVS_API int msvs_index_set_cancel(msvs_index_t * index, int (*is_cancelled)(void * ctx), void * ctx);
/* Finalise: assign rows to lists, lay lists out contiguously (ascending id inside a list), drop staging. */
MSVS_API int msvs_index_build(msvs_index_t * index);
MSVS_API int msvs_index_ready(const msvs_index_t * index);
MSVS_API size_t msvs_index_num_data(const msvs_index_t * index);
MSVS_API size_t msvs_index_num_lists(const msvs_index_t * index);
MSVS_API size_t msvs_index_memory_usage(const msvs_index_t * index);

/* search(): queries nq*dim f32 (HOST); params e.g. "nprobe=32" (IVFFLAT search param, validated like
 * parseVSParameters.cpp:43-222); alive_bits nullable, nbits = number of valid bits; ids/dis nq*k (HOST). */
MSVS_API int msvs_index_search(const msvs_index_t * index, const float * queries, size_t nq, int k,
                               const char * params, const uint64_t * alive_bits, size_t nbits, int64_t * ids,
                               float * dis);
/* Same with DEVICE pointers, enqueued on `hip_stream` (hipStream_t, NULL = default stream) without host
 * synchronisation: the form a GPU-resident host pipeline (and bench.py) uses.  k <= MSVS_MAX_K_ROUNDS; beyond MSVS_MAX_K the
 * call runs the host entry's exact rounds, query by query, stream-ordered like the rest. */
MSVS_API int msvs_index_search_device(const msvs_index_t * index, const float * d_queries, size_t nq, int k,
                                      int nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                      float * d_dis, void * hip_stream);

/* VIWithMeta state of a cached index (src/VectorIndex/Cache/VICacheObject.h:40-117), resident in HBM:
 *  - set_delete_bitmap: the lightweight-delete bitmap (1 = alive, over the index labels), swapped atomically like
 *    VIWithMeta::setDeleteBitmap; every search ANDs it into its filter on the device (VIWithDataPart.cpp:903-908) instead
 *    of the host intersecting and re-uploading bitmaps per query.  NULL clears it.
 *  - set_merged_maps: the row-id maps of a DECOUPLED part (a merged part still served by its source parts' indexes,
 *    SegmentId::getMergedMaps): row_ids_map[label] = row of the merged part; inverted_row_ids_map /
 *    inverted_row_sources_map [merged row] = (label, source part).  Once set, a search takes its filter in the merged
 *    part's row space (getRealBitmap, src/VectorIndex/Utils/VIUtils.cpp:479-498) and reports merged-part rows
 *    (transferToNewRowIds, VIWithDataPart.cpp:56-67). */
MSVS_API int msvs_index_set_delete_bitmap(msvs_index_t * index, const uint64_t * alive_bits, size_t nbits);
MSVS_API int msvs_index_set_merged_maps(msvs_index_t * index, const uint64_t * row_ids_map, size_t n_old,
                                        const uint64_t * inverted_row_ids_map, const uint8_t * inverted_row_sources_map,
                                        size_t n_new, uint32_t own_id);

/* Export the index structure (for parity checks against the oracle and for serialisation):
 * any output may be NULL; sizes: centroids nlist*dim, list_off nlist+1, vecs num_data*dim, ids num_data.
 * Cosine indexes export the stored (normalised) rows. */
MSVS_API int msvs_index_export(const msvs_index_t * index, float * centroids, int64_t * list_off, float * vecs,
                               int64_t * ids);

/* One inverted list of a built IVFFLAT index: its rows (len * dim f32, as stored: cosine indexes hold normalised rows) and
 * labels (len i64), len = list_off[list + 1] - list_off[list] of msvs_index_export.  Lets a checker redo what a few queries
 * touch on an index too large to export whole (12.5M x 1536 = 77 GB).  Either output may be NULL. */
MSVS_API int msvs_index_export_list(const msvs_index_t * index, size_t list, float * vecs, int64_t * ids);

/* Balance of the inverted lists of a built IVFFLAT index: list count, shortest / longest list, and Faiss' imbalance factor
 * nlist * sum(len^2) / n^2 (1 = uniform; the expected number of rows a probe meets is imbalance * n / nlist); train_empty =
 * empty clusters the last k-means iteration had to re-seed (0 for loaded indexes / caller-given centroids).  Any out may be NULL. */
MSVS_API int msvs_index_list_stats(const msvs_index_t * index, size_t * nlist, size_t * min_len, size_t * max_len, double * imbalance,
                                   size_t * train_empty);

/* Serialisation through caller-supplied streams -- the form the reference's library uses: Search::VectorIndex::serialize
 * (IndexDataFileWriter<OS>*) / saveDataID / load(IndexDataFileReader<IS>*) / loadDataID open every file of the index
 * through the host's opener, a VectorIndexWriter / VectorIndexReader over IDisk (local disk or S3 alike):
 * src/VectorIndex/Common/VectorIndexIO.h:25-166, VIWithDataPart.cpp:461-473 and :688-700.
 * The index is a set of NAMED files ("data_bin": header, centroids, list offsets, rows; "id_list": the row ids); the
 * host shim maps NAME to <index_name>-NAME.vidx3 inside the part directory (VICommon.h:55, SegmentId).
 *   open(ctx, name, write) -> stream handle or NULL;  write / read -> bytes moved (a short count is an error / EOF);
 *   close -> 0 on success.  All four are called from the thread that called serialize / load.
 * load validates everything it reads (MSVS_ERR_IO on a corrupt or truncated file; nothing is searched before). */
typedef struct msvs_io
{
    void * ctx;
    void * (*open)(void * ctx, const char * name, int write);
    int64_t (*write)(void * ctx, void * stream, const void * buf, size_t n);
    int64_t (*read)(void * ctx, void * stream, void * buf, size_t n);
    int (*close)(void * ctx, void * stream);
} msvs_io_t;
MSVS_API int msvs_index_serialize_io(const msvs_index_t * index, const msvs_io_t * io);
MSVS_API int msvs_index_load_io(const msvs_io_t * io, msvs_index_t ** out);
/* Convenience over stdio: the file set <path_prefix>-data_bin.vidx3 and <path_prefix>-id_list.vidx3. */
MSVS_API int msvs_index_serialize(const msvs_index_t * index, const char * path_prefix);
MSVS_API int msvs_index_load(const char * path_prefix, msvs_index_t ** out);
/* getVersion().toString() and getResourceUsage() of the reference's index object (VIWithDataPart.cpp:368-385,
 * :485-488): the host records them in <index>-vector_index_description.vidx3 (VIMetadata.cpp:115-187). */
MSVS_API const char * msvs_index_version(void);
MSVS_API int msvs_index_resource_usage(const msvs_index_t * index, size_t * memory_usage_bytes,
                                       size_t * disk_usage_bytes, size_t * build_memory_usage_bytes);

/* Measurement support (bench.py): rows the list scan of msvs_index_search(queries, nprobe) has to look at.
 *   *rows          = sum over (query, probed list) of the list length (the per-query model of SURVEY.md 8d);
 *   *rows_streamed = rows the launch actually streams from HBM given its work decomposition: with query tiles
 *                    of T queries per list pass this is sum over lists of ceil(pairs_on_list / T) * list length
 *                    (== *rows when T == 1).  FLAT: nq * num_data / ceil(nq / T) * num_data;
 *   *rows_unique   = rows probed by at least one query of the batch (the union): what MUST come from HBM at least
 *                    once for this batch, i.e. the batch-level algorithmic bytes / (4d + 4).  Queries are HOST. */
MSVS_API int msvs_index_scanned_rows(const msvs_index_t * index, const float * queries, size_t nq, int nprobe,
                                     uint64_t * rows, uint64_t * rows_streamed, uint64_t * rows_unique);
/* Kernel timing with HIP events recorded on the launch stream around every kernel of the scan path.
 * enable(1) starts collecting, get() synchronises and returns call count and summed milliseconds of the kernel
 * family `name` ("flat_scan", "ivf_scan", "merge", "bm25_score"), reset() drops the samples. */
MSVS_API int msvs_profile_enable(int on);
MSVS_API int msvs_profile_get(const char * name, uint64_t * calls, double * total_ms);
MSVS_API int msvs_profile_reset(void);
/* Counters of the matrix-core candidate pass of batched IVFFLAT searches (many queries per list): `queries` that
 * went through it on the current device since process start and how many of them had no exactness certificate and
 * were re-run through the canonical scan (`fallbacks`).  Results are identical either way; this is a speed metric.
 * Synchronises the device. */
MSVS_API int msvs_prefilter_stats(uint64_t * queries, uint64_t * fallbacks);
/* ... and of the coarse quantiser's candidate passes (whose output is the probe lists). */
MSVS_API int msvs_coarse_stats(uint64_t * queries, uint64_t * fallbacks);
/* msvs_index_search from many host threads (the reference: one query per thread, up to ScanThreadLimiter of them,
 * MergeTreeVSManager.cpp:973): up to 8 unfiltered calls of <= 4 queries run directly; callers beyond that queue, and the next call
 * to finish hands its slot to the first waiter together with every waiter that asks for the same k and parameters -- one batched
 * search serves them all (same bits: every path is exact).  Counters: calls through this front end, batches of several callers,
 * queries served by such batches.  Option "combine" = the number of direct calls (0: off). */
MSVS_API int msvs_combine_stats(uint64_t * calls, uint64_t * batches, uint64_t * batched_queries);
/* Scratch memory is kept per (host thread, stream) and reused call after call; it shrinks by itself when a thread's
 * requests stay small for a window of 64 calls.  msvs_release_scratch frees the calling thread's arenas now (device synchronised). */
MSVS_API int msvs_release_scratch(size_t * freed_bytes);
/* Experiment / test knobs (DESIGN.md section 6b lists them; none is needed in production).  They are read ONCE per
 * process from the MSVS_<NAME> environment variables; afterwards only this call changes them -- a search never calls
 * getenv.  `name` without the MSVS_ prefix, any case; value NULL or "" restores the default.
 * MSVS_ERR_INVALID_ARGUMENT for an unknown name. */
MSVS_API int msvs_set_option(const char * name, const char * value);

/* Multi-GPU: one process per GPU, every process holds ONE shard of the index (msvs_index_create params
 * shard_rank / shard_world: IVF lists list_id % world, FLAT row ranges; centroids replicated) and a communicator.
 * msvs_shard_search_device is the whole sharded search as ONE stream-ordered call: the coarse quantiser sharded by
 * query + one all-gather of the probe lists, the scan of the local lists, one all-gather of the packed partial top-k
 * (nq * k * 12 B per rank over xGMI) and the canonical W-way merge -- the device-side analogue of the per-part searches
 * + getTotalTopSearchResultImpl (MergeTreeBaseSearchManager.cpp:207-299).  Every rank calls it with the SAME queries
 * and gets the SAME result (ids bit-exact with the unsharded index).
 * The communicator is RCCL (librccl resolved at first use, straight rccl.h calls): rank 0 creates the id
 * (msvs_comm_unique_id), the host distributes its MSVS_COMM_ID_BYTES bytes by any means it has (ClickHouse: its own
 * TCP / Keeper), every rank calls msvs_comm_init on its device.  msvs_comm_init_custom plugs a caller-supplied
 * all-gather instead (tests run two ranks on one GPU over gloo): it must gather `bytes` from d_send of every rank into
 * d_recv[rank * bytes ...] of every rank, ordered after the work already enqueued on `hip_stream`, and return 0. */
#define MSVS_COMM_ID_BYTES 128
typedef struct msvs_comm msvs_comm_t;
typedef int (*msvs_allgather_fn)(void * ctx, const void * d_send, void * d_recv, size_t bytes, void * hip_stream);
MSVS_API int msvs_comm_unique_id(void * id_out /* MSVS_COMM_ID_BYTES */);
MSVS_API int msvs_comm_init(const void * id, int nranks, int rank, msvs_comm_t ** out);
MSVS_API int msvs_comm_init_custom(int nranks, int rank, msvs_allgather_fn all_gather, void * ctx, msvs_comm_t ** out);
MSVS_API void msvs_comm_free(msvs_comm_t * comm);
/* Sum of n u64 counters over the ranks, in place in HOST memory, every rank gets the sums -- the one exchange step of a sharded
 * BM25 search: (total documents, total tokens per column, document frequency per query term), what BM25InfoInDataParts /
 * the ftsIndex table function add up over parts and shards (BM25InfoInDataParts.cpp:40-93, StorageFtsIndex.cpp:150-213).
 * Runs on the communicator's all-gather (RCCL or the caller's), ordered on hip_stream, and returns when the sums are there. */
MSVS_API int msvs_comm_all_reduce_u64(const msvs_comm_t * comm, uint64_t * values, size_t n, void * hip_stream);
MSVS_API int msvs_comm_rank(const msvs_comm_t * comm);
MSVS_API int msvs_comm_size(const msvs_comm_t * comm);
/* (The sharded and routed searches keep k <= MSVS_MAX_K: no rounds across ranks.) */
MSVS_API int msvs_shard_search_device(const msvs_index_t * shard, const msvs_comm_t * comm, const float * d_queries,
                                      size_t nq, int k, int nprobe, const uint64_t * d_alive_bits, size_t nbits,
                                      int64_t * d_ids, float * d_dis, void * hip_stream);
/* The ROUTED form: every rank brings its OWN batch (nq may differ per rank, 0 included) and gets the results of its own queries -- the
 * queries that arrived at this server, StorageDistributed.cpp:1213-1255 -- instead of every rank working through the same batch.
 * FRONT phase: a query's coarse quantiser and the pre-pruning by the list radius (over the lists of the whole index) run on its home
 * rank; one all-gather of the rank x rank count matrix (+ a header per rank: status, filter / pruning flags, shard instance, k, nprobe)
 * is read by every host.  BACK phase: the query visits only the ranks that own lists it still needs (ncclSend / ncclRecv of the exact
 * sizes, grouped), each of which searches it under ITS OWN filter -- d_alive_bits (nullable; 1 = row may be returned, over the row ids
 * this rank holds, like msvs_index_search_device) AND the shard's resident delete bitmap (VIWithDataPart.cpp:903-908) -- and returns
 * the exact top-k over its lists; the home rank merges (MergeTreeBaseSearchManager.cpp:207-299) and applies its row-id map.  ids and
 * distances == the unsharded index's under the union of the filters, bit for bit.  IVFFLAT shards, <= 32 ranks.
 * COLLECTIVE: every rank of the communicator calls it for every step with the same k and nprobe.  What goes wrong on ONE rank before
 * the exchange (bad argument, unsupported k, allocation failure, index not ready, mismatching k / nprobe) is published in the matrix:
 * EVERY rank returns an error for that step and none blocks.  A shard object replaced on one rank (reloaded part) is noticed through
 * its instance word and the index-wide list statistics are gathered again by every rank in the same step.
 * routed_pairs (nullable): the (query, rank) pairs this rank served -- its share of the step's list-scan work.  A caller-supplied
 * transport (msvs_comm_init_custom) emulates the point-to-point exchange with its all-gather (tests). */
MSVS_API int msvs_shard_search_routed_device(const msvs_index_t * shard, const msvs_comm_t * comm, const float * d_queries, size_t nq,
                                             int k, int nprobe, int64_t * d_ids, float * d_dis, void * hip_stream, uint64_t * routed_pairs);
MSVS_API int msvs_shard_search_routed_filtered_device(const msvs_index_t * shard, const msvs_comm_t * comm, const float * d_queries,
                                                      size_t nq, int k, int nprobe, const uint64_t * d_alive_bits, size_t nbits,
                                                      int64_t * d_ids, float * d_dis, void * hip_stream, uint64_t * routed_pairs);
/* The routed search with TWO STEPS IN FLIGHT: call i enqueues the FRONT phase of its batch and then the BACK phase of batch i - 1,
 * whose count matrix was gathered one call ago -- the host does not wait for the device while the list scan of step i - 1 and the
 * coarse stage of step i are still to run.  Both phases run in `hip_stream`'s order (option route_streams = 2: on the communicator's
 * own compute + exchange streams, `hip_stream` ordering the inputs only); a call on another stream than the previous one continues
 * behind it.  The results (and *routed_pairs) of batch i are complete when call i + 1's work on its stream is -- or when the event
 * handed out by call i + 1 in *prev_done_event has fired (prev_done_event may be NULL: no event is recorded then; nullptr at the
 * first call) -- or after msvs_shard_search_drain, which is COLLECTIVE while a routed step is pending (it runs that step's back
 * phase).  Buffers of a batch stay untouched until then; every rank issues the same sequence of calls. */
MSVS_API int msvs_shard_search_routed_device_async(const msvs_index_t * shard, const msvs_comm_t * comm, const float * d_queries, size_t nq,
                                                   int k, int nprobe, const uint64_t * d_alive_bits, size_t nbits, int64_t * d_ids,
                                                   float * d_dis, void * hip_stream, uint64_t * routed_pairs, void ** prev_done_event);
/* The same search with TWO BATCHES IN FLIGHT: the call returns once batch i is enqueued; `hip_stream` orders its INPUTS only,
 * its results are complete when *done_event -- a hipEvent_t owned by the communicator, valid until the second-next async call on
 * it -- has fired: hipStreamWaitEvent on whatever stream reads d_ids / d_dis, or msvs_shard_search_drain.  The coarse pass and
 * the list scan run on the communicator's compute stream, both all-gathers and the merge on its exchange stream, so the packed
 * top-k exchange + merge of batch i (latency-bound: tens of microseconds over xGMI) hide under the list scan of batch i + 1 --
 * the per-part searches of MergeTreeBaseSearchManager.cpp:207-299 overlapping with the merge of the previous query.  d_queries,
 * d_ids, d_dis of a batch must stay untouched until its event; every rank issues the same sequence of calls. */
MSVS_API int msvs_shard_search_device_async(const msvs_index_t * shard, const msvs_comm_t * comm, const float * d_queries,
                                            size_t nq, int k, int nprobe, const uint64_t * d_alive_bits, size_t nbits,
                                            int64_t * d_ids, float * d_dis, void * hip_stream, void ** done_event);
/* `hip_stream` waits for every batch still in flight on the communicator. */
MSVS_API int msvs_shard_search_drain(const msvs_comm_t * comm, void * hip_stream);

/* Multi-part / multi-GPU merge of partial top-k lists with the canonical total order -- the
 * device-side analogue of MergeTreeBaseSearchManager::getTotalTopSearchResultImpl
 * (src/VectorIndex/Storages/MergeTreeBaseSearchManager.cpp:207-299) for lists that share one id space.
 * ids/dis: [nparts][nq][k] (HOST), out: [nq][k].
 *   metric: MSVS_METRIC_L2 (ascending distances; also for cosine distances) or MSVS_METRIC_IP (descending), anything else
 *   MSVS_ERR_NOT_IMPLEMENTED; k <= MSVS_MAX_K (MSVS_ERR_UNSUPPORTED_K); nq = 0 or k = 0 is a no-op; nparts = 0 writes nq * k empty slots.
 *   An entry counts when its id is >= 0 and its distance is strictly better than the neutral value: < FLT_MAX, IP: > -FLT_MAX,
 *   never NaN.  Order: the distance as a FLOAT (-0 and +0 tie; a -0 is reported as +0), then the ascending id; every copy of a
 *   (distance, id) that several parts hold keeps a slot.  Unfilled slots: id -1 at the neutral value.
 *   Ids lie in [0, 2^32 - 1) like every id of the library (the keys carry 32 bits).  msvs_merge_topk refuses a larger one with
 *   MSVS_ERR_ID_RANGE; the device forms cannot look without a synchronisation and return such an id truncated.
 *   PRECONDITION: every part's [k] list is in that order, best first, with its entries that do not count (id -1) at the END --
 *   what every search entry writes.  Between 257 and 6144 keys per query the merge walks the lists from their heads and relies
 *   on it; the result for other input is unspecified (never out of bounds). */
MSVS_API int msvs_merge_topk(const int64_t * ids, const float * dis, size_t nparts, size_t nq, size_t k, int metric,
                             int64_t * out_ids, float * out_dis);
MSVS_API int msvs_merge_topk_device(const int64_t * d_ids, const float * d_dis, size_t nparts, size_t nq, size_t k,
                                    int metric, int64_t * d_out_ids, float * d_out_dis, void * hip_stream);
/* Same, but shard p's [nq][k] lists start at d_ids + p * ids_part_stride / d_dis + p * dis_part_stride (strides in
 * ELEMENTS): lets each rank all-gather ONE packed buffer {ids[nq*k] i64 | dis[nq*k] f32} and merge it in place. */
MSVS_API int msvs_merge_topk_device_strided(const int64_t * d_ids, size_t ids_part_stride, const float * d_dis,
                                            size_t dis_part_stride, size_t nparts, size_t nq, size_t k, int metric,
                                            int64_t * d_out_ids, float * d_out_dis, void * hip_stream);

/* Fusion step of a hybrid search for a batch, on the device: RankFusion / RelativeScoreFusion / computeNormalizedScore
 * (src/VectorIndex/Utils/HybridSearchUtils.cpp:164-300) as MergeTreeHybridSearchManager::hybridSearch applies them to ONE
 * part's vector and text results.  Inputs are the device searches' output arrays: query q's vector rows d_vec_dis /
 * d_vec_ids[q * kv ...] (best first; the first id < 0 ends the list), its text rows d_txt_scores / d_txt_ids[q * kt ...];
 * kv, kt, topk <= MSVS_MAX_K_ROUNDS (lists of at most 256 rows: every entry compares itself with every other; longer ones: a hash
 * table of the text labels and a sort of the fused rows, one workgroup per query either way).  fusion_type: 0 = RRF (score = sum of 1 / (fusion_k + rank), fusion_k 0 = 60), 1 = RSF (fusion_weight *
 * normalised text score + (1 - fusion_weight) * normalised vector score, vector_scan_direction -1: larger is better).
 * Outputs [nq][topk]: fused scores descending, ties by ascending label; label -1 / score +0 past d_n_out[q] rows.  Same
 * arithmetic, same order, same bits as msvs_host_hybrid_search_batch (include/msvs_host.h).  Stream-ordered, no host sync.
 * NaN fused scores: RSF normalises with (s - min) / (max - min), so a +inf distance at the head of an otherwise finite list
 * (an overflowing row under inner product) or a NaN handed in gives a NaN fused score.  A row whose fused score is NaN ranks
 * behind every row whose score is not NaN; NaN rows among themselves are ordered by ascending label; they count in d_n_out
 * like any other row.
 * Precondition: each list holds distinct labels (the row ids of one search).  For a list with a repeated label the result is
 * unspecified, but every access stays in bounds. */
MSVS_API int msvs_hybrid_fuse_device(int fusion_type, const float * d_vec_dis, const int64_t * d_vec_ids, size_t kv,
                                     const float * d_txt_scores, const int64_t * d_txt_ids, size_t kt, size_t nq,
                                     uint64_t fusion_k, float fusion_weight, int vector_scan_direction, size_t topk,
                                     float * d_out_scores, int64_t * d_out_labels, uint32_t * d_n_out, void * hip_stream);

/* ---------------------------------------------------------------------------------------------
 * Seam B -- BM25 posting-list scorer.  Replaces the scoring inside
 *   TANTIVY::ffi_bm25_search(index_path, sentence, column_names, topk, alive_bitmap, use_filter, enable_nlq,
 *                            operator_or, statistics)   src/Storages/MergeTree/TantivyIndexStore.cpp:908-917,939-948
 * Tokenisation / query parsing stay on the host; the postings of a part are exported once into flat arrays:
 * term t owns postings [post_off[t], post_off[t+1]) of (doc_ids ascending, tfs); fieldnorm_ids[doc] is
 * tantivy's 1-byte quantised field length.
 */
typedef struct msvs_postings msvs_postings_t;
MSVS_API int msvs_postings_create(const int64_t * post_off, size_t num_terms, const uint32_t * doc_ids,
                                  const uint32_t * tfs, const uint8_t * fieldnorm_ids, size_t num_docs,
                                  msvs_postings_t ** out);
/* Several text columns in one index (fts index on (doc, doc2): TantivyIndexStore passes column_names): every
 * (field, token) pair is a term of its own with term_field[t] = its field; fieldnorm_ids is [num_fields][num_docs].
 * num_fields <= 4. */
MSVS_API int msvs_postings_create_fields(const int64_t * post_off, size_t num_terms, const uint8_t * term_field,
                                         const uint32_t * doc_ids, const uint32_t * tfs, const uint8_t * fieldnorm_ids,
                                         size_t num_fields, size_t num_docs, msvs_postings_t ** out);
MSVS_API void msvs_postings_free(msvs_postings_t * postings);
/* The part's lightweight-delete bitmap (1 = alive; what MergeTreeTextSearchManager.cpp:199-255 hands to tantivy as
 * u8_alive_bitmap on every call), resident in HBM and swapped atomically; NULL clears.  A per-call filter is ANDed in. */
MSVS_API int msvs_postings_set_alive(msvs_postings_t * postings, const uint64_t * alive_bits, size_t nbits);
/* qterms/df: the query's term ids and their TABLE-level document frequencies (TANTIVY::Statistics.docs_freq,
 * src/VectorIndex/Processors/ReadWithHybridSearch.cpp:89-209); total_docs / total_tokens likewise.
 * Output: up to k (row id, score) best-first (score desc, row asc); *n_out = number written.  k <= MSVS_MAX_K_ROUNDS (all
 * BM25 entries; beyond MSVS_MAX_K: exact rounds of MSVS_MAX_K ranks over the whole batch, each continuing behind the last
 * (score, row) of the one before). */
MSVS_API int msvs_bm25_search(const msvs_postings_t * postings, const uint32_t * qterms, const uint64_t * df,
                              size_t num_qterms, uint64_t total_docs, uint64_t total_tokens,
                              const uint64_t * alive_bits, size_t nbits, size_t k, uint64_t * row_ids, float * scores,
                              size_t * n_out);
/* A BATCH of nq queries in one pass (one query is far too little work for the chip: a few MB of postings).
 * Query q owns the flat terms [qoff[q], qoff[q + 1]) of qterms / df (table-level document frequency of each
 * (field, token) term) / qgroups (nullable: the index of the query TOKEN a term stands for -- a token searched in two
 * fields is two terms of one group; NULL = every term its own group).  total_tokens: [num_fields].
 * operator_or != 0: any term matches (tantivy's default, ffi_bm25_search(..., operator_or = true)); 0: every token
 * group must match (at most 16 tokens).  Outputs [nq][k] best-first (score desc, row asc), n_out[q] = hits of query q.
 * The _device form leaves int64 ids (-1 = no hit) and scores in device buffers, stream-ordered, no host sync; its filter
 * is a DEVICE pointer. */
MSVS_API int msvs_bm25_search_batch(const msvs_postings_t * postings, size_t nq, const uint32_t * qoff,
                                    const uint32_t * qterms, const uint32_t * qgroups, const uint64_t * df,
                                    uint64_t total_docs, const uint64_t * total_tokens, int operator_or,
                                    const uint64_t * alive_bits, size_t nbits, size_t k, uint64_t * row_ids, float * scores,
                                    uint32_t * n_out);
/* ---------------------------------------------------------------------------------------------- filters (PREWHERE)
 * The reference evaluates PREWHERE with a CPU pipeline per query and part, collects the passing `_part_offset`s and
 * sets one bit per row (performPrefilter / getFilterFromPipeline,
 * src/VectorIndex/Storages/MergeTreeSelectWithHybridSearchProcessor.cpp:905-1112); the bitmap then rides on the search
 * (executeSearchWithFilter).  msvs_filter_t is that bitmap, resident on the device, with its population count:
 *   - built from host / device words, from a list of passing row offsets (exactly getFilterFromPipeline's loop), or from a
 *     simple predicate `column OP constant` evaluated on the device (row i of the column = `_part_offset` i);
 *   - combined with AND / OR / AND NOT;
 *   - handed to msvs_index_search_filter*, which picks the strategy: bit test inside the scan, or -- when few rows pass
 *     (below 3 % .. 40 % depending on how many queries share a list pass) -- the scan of a compacted view holding only the
 *     passing rows (same results, a fraction of the bytes).  Results are identical to msvs_index_search with the same bitmap. */
typedef struct msvs_filter msvs_filter_t;
/* The predicate compares VALUES, as SQL does: the constant is never cast into the column type (UInt8 `< 300` passes every row,
 * unsigned `> -1` every row, UInt64 rows >= 2^63 are above every .i), and Float32 rows are compared with .f in double. */
typedef struct { int64_t i; double f; } msvs_scalar_t; /* .i for integer columns, .f for float columns */
enum msvs_dtype { MSVS_DT_UINT8 = 0, MSVS_DT_UINT16, MSVS_DT_UINT32, MSVS_DT_UINT64, MSVS_DT_INT8, MSVS_DT_INT16, MSVS_DT_INT32,
                  MSVS_DT_INT64, MSVS_DT_FLOAT32, MSVS_DT_FLOAT64 };
enum msvs_cmp_op { MSVS_OP_EQ = 0, MSVS_OP_NE, MSVS_OP_LT, MSVS_OP_LE, MSVS_OP_GT, MSVS_OP_GE, MSVS_OP_BETWEEN /* lo <= x <= hi */ };
enum msvs_filter_mode { MSVS_FILTER_AND = 0, MSVS_FILTER_OR = 1, MSVS_FILTER_AND_NOT = 2 };
MSVS_API int msvs_filter_from_bits(const uint64_t * bits, size_t nbits, msvs_filter_t ** out);
MSVS_API int msvs_filter_from_offsets(const uint64_t * part_offsets, size_t n, size_t nbits, int mem, msvs_filter_t ** out);
MSVS_API int msvs_filter_from_predicate(const void * column, int dtype, size_t nrows, int mem, int op, msvs_scalar_t lo,
                                        msvs_scalar_t hi, msvs_filter_t ** out);
MSVS_API int msvs_filter_combine(msvs_filter_t * a, const msvs_filter_t * b, int mode); /* a = a MODE b; a keeps its length,
                                                                                           b is zero-extended or cut to it */
MSVS_API int msvs_filter_count(const msvs_filter_t * f, uint64_t * alive, size_t * nbits);
MSVS_API int msvs_filter_to_bits(const msvs_filter_t * f, uint64_t * bits_out);
MSVS_API void msvs_filter_free(msvs_filter_t * f);
MSVS_API int msvs_index_search_filter(const msvs_index_t * index, const float * queries, size_t nq, int k, const char * params,
                                      const msvs_filter_t * filter, int64_t * ids, float * dis);
/* (both: k <= MSVS_MAX_K_ROUNDS; beyond MSVS_MAX_K exact rounds over the filter's bit test, as msvs_index_search) */
MSVS_API int msvs_index_search_filter_device(const msvs_index_t * index, const float * d_queries, size_t nq, int k, int nprobe,
                                             const msvs_filter_t * filter, int64_t * d_ids, float * d_dis, void * hip_stream);

/* Monitoring: queries scored through the sample / cut / emit path of long corpora, and how many of them needed the
 * exact fallback (speed only; results never differ). */
MSVS_API int msvs_bm25_stats(uint64_t * queries, uint64_t * fallbacks);
MSVS_API int msvs_bm25_search_batch_device(const msvs_postings_t * postings, size_t nq, const uint32_t * qoff,
                                           const uint32_t * qterms, const uint32_t * qgroups, const uint64_t * df,
                                           uint64_t total_docs, const uint64_t * total_tokens, int operator_or,
                                           const uint64_t * d_alive_bits, size_t nbits, size_t k, int64_t * d_row_ids,
                                           float * d_scores, void * hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MSVS_H */
