/*
 * msvs_oracle.c -- CPU ORACLE for the MyScaleDB vector-scan / BM25 hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may call it.  The product (libmsvs.so) never links,
 * loads or falls back to anything in oracle/.
 *
 * It is a plain-C restatement of the reference's algorithm for the path
 *   distance()/batch_distance() -> MergeTreeVSManager -> VIWithColumnInPart::search /
 *   searchWithoutIndex -> tryBruteForceSearch -> faiss::knn_L2sqr / knn_inner_product
 * and TextSearch()/HybridSearch() -> TantivyIndexStore::bm25Search -> ffi_bm25_search.
 * File:line citations are relative to /root/reference/.
 *
 * The arithmetic itself lives in two absent third-party submodules
 * (contrib/search-index [bundles Faiss], rust/supercrate/libs/tantivy_search
 * [tantivy 0.21.1, Cargo.lock:2078-2079]; .gitmodules:338-343, commits unpinned),
 * so the oracle restates their PUBLISHED algorithms and is pinned against the
 * reference's own golden outputs (the .reference files under tests/queries/2_vector_search; see
 * tests/golden/ and tests/test_oracle_golden.py).
 *
 * What the goldens pin (verified in tests/test_oracle_golden.py):
 *   - L2 is returned SQUARED, computed by direct difference in f32 with SEPARATELY
 *     ROUNDED multiply and add (no FMA): 00001 (25.230003 -- an fma chain gives
 *     25.230001), 00012, 00002.
 *   - IP likewise mul-then-add (00002: 29.400002; fma gives 29.4).
 *   - cosine = 1 - <x^,y^> with x^ = x / sqrt(sum x^2), the norm accumulated
 *     SEQUENTIALLY (VectorDataset.h:98-117) and the inner product accumulated as a
 *     SIMD-style tree ((p0+p1)+(p2+p3) for d=4: 00014_*_ivfflat/hnsw goldens match
 *     10/10 only with that order; a sequential IP matches 7/10).
 * What they do not pin: the accumulation order for d > 4 (the 768-d goldens of 00028
 * agree to print precision with every order) and tie-breaking among equal distances.
 * We therefore FIX one canonical order, used identically by this oracle and by the HIP
 * kernels, so that distances are bit-identical and ids can be compared bit-exact:
 *
 *   CANONICAL DOT/L2 ORDER ("W64 tree"):
 *     acc[i] = 0 for i in 0..63
 *     for k = 0..d-1 (ascending):  acc[k % 64] = acc[k % 64] + p_k      (f32, rounded)
 *        with p_k = fl(fl(x_k - y_k) * fl(x_k - y_k))   (L2)
 *          or p_k = fl(x_k * y_k)                        (IP)
 *     then a pairwise adjacent tree in index order:
 *        for s in 1,2,4,8,16,32: for i multiple of 2s: acc[i] = acc[i] + acc[i+s]
 *     result = acc[0]
 *   (This is the 64-lane generalisation of Faiss' fvec_* SIMD loops: strided partial
 *   sums followed by a horizontal-add tree; for d <= 4 it is exactly the SSE hadd tree.)
 *
 *   CANONICAL TOP-K ORDER: L2/cosine ascending (dist, id); IP descending dist then
 *   ascending id.  A candidate is admitted only if strictly better than the heap's
 *   neutral value (L2: d < FLT_MAX; IP: ip > -FLT_MAX; NaN never) -- the public Faiss
 *   CMax/CMin heap semantics behind BruteForceSearch.h:80-88.  Unfilled slots: id -1,
 *   distance = neutral.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORACLE_API __attribute__((visibility("default")))

enum { METRIC_L2 = 0, METRIC_IP = 1, METRIC_COSINE = 2 };

/* ------------------------------------------------------------------ distances */

static inline float tree64(float *acc)
{
    for (int s = 1; s < 64; s <<= 1)
        for (int i = 0; i < 64; i += 2 * s)
            acc[i] = acc[i] + acc[i + s];
    return acc[0];
}

ORACLE_API float oracle_l2sqr(const float *x, const float *y, size_t d)
{
    float acc[64];
    for (int i = 0; i < 64; i++) acc[i] = 0.0f;
    size_t k = 0;
    for (; k + 64 <= d; k += 64)
        for (int i = 0; i < 64; i++) {
            float t = x[k + i] - y[k + i];
            float p = t * t;
            acc[i] = acc[i] + p;
        }
    for (int i = 0; k < d; k++, i++) {
        float t = x[k] - y[k];
        float p = t * t;
        acc[i] = acc[i] + p;
    }
    return tree64(acc);
}

ORACLE_API float oracle_ip(const float *x, const float *y, size_t d)
{
    float acc[64];
    for (int i = 0; i < 64; i++) acc[i] = 0.0f;
    size_t k = 0;
    for (; k + 64 <= d; k += 64)
        for (int i = 0; i < 64; i++) {
            float p = x[k + i] * y[k + i];
            acc[i] = acc[i] + p;
        }
    for (int i = 0; k < d; k++, i++) {
        float p = x[k] * y[k];
        acc[i] = acc[i] + p;
    }
    return tree64(acc);
}

/* VectorDataset<FloatVector>::normalize(), src/VectorIndex/Common/VectorDataset.h:98-117:
 * sequential f32 sum of squares, rows with sum < FLT_EPSILON are left untouched,
 * otherwise every element is divided by sqrt(sum). */
ORACLE_API void oracle_normalize_rows(float *x, size_t n, size_t d)
{
    for (size_t r = 0; r < n; r++) {
        float *p = x + r * d;
        float sum = 0;
        for (size_t j = 0; j < d; j++) {
            float sq = p[j] * p[j];
            sum = sum + sq;
        }
        if (sum < FLT_EPSILON) continue;
        sum = sqrtf(sum);
        for (size_t j = 0; j < d; j++) p[j] = p[j] / sum;
    }
}

/* ------------------------------------------------------------------ top-k */

typedef struct {
    float dis;
    int64_t id;
} cand_t;

/* returns 1 if a is strictly better than b under the canonical order */
static inline int better(int metric, float da, int64_t ia, float db, int64_t ib)
{
    if (metric == METRIC_IP) {
        if (da > db) return 1;
        if (da < db) return 0;
    } else {
        if (da < db) return 1;
        if (da > db) return 0;
    }
    return ia < ib;
}

static inline float neutral(int metric) { return metric == METRIC_IP ? -FLT_MAX : FLT_MAX; }

static inline int admissible(int metric, float d)
{
    return metric == METRIC_IP ? (d > -FLT_MAX) : (d < FLT_MAX);
}

/* sorted insertion into a best-first array of length k (cnt filled) */
static void topk_push(int metric, cand_t *h, size_t k, size_t *cnt, float d, int64_t id)
{
    if (!admissible(metric, d)) return;
    if (*cnt == k) {
        if (k == 0 || !better(metric, d, id, h[k - 1].dis, h[k - 1].id)) return;
    } else {
        (*cnt)++;
    }
    size_t j = *cnt - 1;
    while (j > 0 && better(metric, d, id, h[j - 1].dis, h[j - 1].id)) {
        h[j] = h[j - 1];
        j--;
    }
    h[j].dis = d;
    h[j].id = id;
}

static inline int bit_alive(const uint64_t *bits, size_t i)
{
    return bits == NULL || ((bits[i >> 6] >> (i & 63)) & 1);
}

/*
 * Exact k-NN of nx queries against ny base rows: the restatement of
 * tryBruteForceSearch<FloatVector> (src/VectorIndex/Common/BruteForceSearch.h:63-92)
 * -> faiss::knn_L2sqr (maxheap) / faiss::knn_inner_product (minheap), results sorted
 * best-first, unfilled slots id -1 (host tests `> -1`, MergeTreeVSManager.cpp:1507,1523).
 * metric: METRIC_L2 or METRIC_IP.  labels (nullable): id of row i, else i.
 * alive (nullable): LSB-first u64 bitmap over base rows, 1 = candidate.
 */
ORACLE_API int oracle_knn(const float *x, const float *y, size_t d, size_t k, size_t nx, size_t ny, int metric,
                          const int64_t *labels, const uint64_t *alive, int64_t *ids, float *dis)
{
    if (metric != METRIC_L2 && metric != METRIC_IP) return 2; /* NOT_IMPLEMENTED, BruteForceSearch.h:89-92 */
    cand_t *h = (cand_t *)malloc(sizeof(cand_t) * (k ? k : 1));
    for (size_t q = 0; q < nx; q++) {
        size_t cnt = 0;
        const float *xq = x + q * d;
        for (size_t i = 0; i < ny; i++) {
            if (!bit_alive(alive, i)) continue;
            float v = metric == METRIC_IP ? oracle_ip(xq, y + i * d, d) : oracle_l2sqr(xq, y + i * d, d);
            topk_push(metric, h, k, &cnt, v, labels ? labels[i] : (int64_t)i);
        }
        for (size_t j = 0; j < k; j++) {
            ids[q * k + j] = j < cnt ? h[j].id : -1;
            dis[q * k + j] = j < cnt ? h[j].dis : neutral(metric);
        }
    }
    free(h);
    return 0;
}

/*
 * Binary vectors (FixedString(N), dimension = 8 N bits): the restatement of tryBruteForceSearch<BinaryVector>
 * (src/VectorIndex/Common/BruteForceSearch.h:94-110) -> faiss::hammings_knn_mc / jaccard_knn.
 *   metric 3 (Hamming): popcount(x xor y), reported as a float (the goldens print 4, 8, 12 ...);
 *   metric 4 (Jaccard): (|x or y| - |x and y|) / |x or y| as ONE f32 division of the two exact counts (Faiss'
 *     JaccardComputer; the goldens' 0.22222222 and 0.33333334 are f32(4/18) and f32(1/3) -- `1 - f32(14/18)` would
 *     print 0.2222222), 1.0 when both vectors are all zero.
 * Results ascending by (distance, id) (the reference's tests order ties by id themselves:
 * tests/queries/2_vector_search/00038_mqvs_binary_vector_feature.sql), unfilled slots id -1 / FLT_MAX.
 * alive (nullable): LSB-first bitmap over the base rows.
 */
enum { METRIC_HAMMING = 3, METRIC_JACCARD = 4 };

ORACLE_API int oracle_knn_bin(const uint8_t *x, const uint8_t *y, size_t nbytes, size_t k, size_t nx, size_t ny, int metric,
                              const uint64_t *alive, int64_t *ids, float *dis)
{
    if (metric != METRIC_HAMMING && metric != METRIC_JACCARD) return 2; /* NOT_IMPLEMENTED, BruteForceSearch.h:106-109 */
    cand_t *h = (cand_t *)malloc(sizeof(cand_t) * (k ? k : 1));
    for (size_t q = 0; q < nx; q++) {
        size_t cnt = 0;
        const uint8_t *xq = x + q * nbytes;
        for (size_t i = 0; i < ny; i++) {
            if (!bit_alive(alive, i)) continue;
            const uint8_t *yi = y + i * nbytes;
            uint32_t ham = 0, num = 0, den = 0;
            for (size_t b = 0; b < nbytes; b++) {
                ham += (uint32_t)__builtin_popcount((unsigned)(xq[b] ^ yi[b]));
                num += (uint32_t)__builtin_popcount((unsigned)(xq[b] & yi[b]));
                den += (uint32_t)__builtin_popcount((unsigned)(xq[b] | yi[b]));
            }
            float v = metric == METRIC_HAMMING ? (float)ham : (den == 0 ? 1.0f : (float)(den - num) / (float)den);
            topk_push(METRIC_L2, h, k, &cnt, v, (int64_t)i);
        }
        for (size_t j = 0; j < k; j++) {
            ids[q * k + j] = j < cnt ? h[j].id : -1;
            dis[q * k + j] = j < cnt ? h[j].dis : FLT_MAX;
        }
    }
    free(h);
    return 0;
}

/*
 * VIWithColumnInPart::searchWithoutIndex<FloatVector> (src/VectorIndex/Common/VIWithDataPart.h:341-382):
 * cosine => normalize() BOTH datasets IN PLACE, search with IP, then d = 1 - d for all
 * k*nq slots (including unfilled ones).  x and y are modified when metric is cosine,
 * exactly as in the reference.
 */
ORACLE_API int oracle_search_without_index(float *x, float *y, size_t d, size_t k, size_t nx, size_t ny, int metric,
                                           const uint64_t *alive, int64_t *ids, float *dis)
{
    int m = metric;
    if (metric == METRIC_COSINE) {
        m = METRIC_IP;
        oracle_normalize_rows(x, nx, d);
        oracle_normalize_rows(y, ny, d);
    }
    int rc = oracle_knn(x, y, d, k, nx, ny, m, NULL, alive, ids, dis);
    if (rc) return rc;
    if (metric == METRIC_COSINE)
        for (size_t i = 0; i < k * nx; i++) dis[i] = 1 - dis[i];
    return 0;
}

/*
 * MergeTreeVSManager::searchWrapper<FloatVector> (src/VectorIndex/Storages/MergeTreeVSManager.cpp:1537-1679):
 * one brute-force block against the running (final_id, final_distance) of size nq*k.
 *  - sentinels: IP -> numeric_limits<float>::min() (FLT_MIN, smallest positive normal!), else FLT_MAX (:1560-1575)
 *  - delete_id_num > 0: over-fetch k+delete_id_num, drop rows whose bit in row_exists is 0 (:1612-1633)
 *  - prewhere: map block-local ids through actual_id_in_range (:1642-1650)
 *  - 2-way merge, strict compare so the running (earlier) entry wins ties; ids get + num_rows_read (:1652-1678)
 * base (and query, for cosine) are normalised in place like the reference.
 */
ORACLE_API int oracle_search_wrapper(int prewhere, float *query, float *base, size_t nbase, int k, int dim, int nq,
                                     int num_rows_read, int64_t *final_id, float *final_distance,
                                     const uint64_t *actual_id_in_range, int metric, const uint64_t *row_exists,
                                     int delete_id_num)
{
    float sentinel = metric == METRIC_IP ? FLT_MIN : FLT_MAX;
    size_t kk = (size_t)k + (size_t)(delete_id_num > 0 ? delete_id_num : 0);
    float *per_distance = (float *)malloc(sizeof(float) * k * nq);
    int64_t *per_id = (int64_t *)malloc(sizeof(int64_t) * k * nq);
    for (int i = 0; i < k * nq; i++) {
        per_distance[i] = sentinel;
        per_id[i] = -1;
    }
    int rc;
    if (delete_id_num > 0) {
        float *tmp_d = (float *)malloc(sizeof(float) * kk * nq);
        int64_t *tmp_i = (int64_t *)malloc(sizeof(int64_t) * kk * nq);
        rc = oracle_search_without_index(query, base, dim, kk, nq, nbase, metric, NULL, tmp_i, tmp_d);
        for (int i = 0; i < nq && !rc; i++) {
            size_t cur = 0, t = 0;
            while (cur < (size_t)k && t < kk) {
                int64_t id = tmp_i[i * kk + t];
                if (id >= 0 && bit_alive(row_exists, (size_t)id)) {
                    per_id[i * k + cur] = id;
                    per_distance[i * k + cur] = tmp_d[i * kk + t];
                    cur++;
                }
                t++;
            }
        }
        free(tmp_d);
        free(tmp_i);
    } else {
        rc = oracle_search_without_index(query, base, dim, k, nq, nbase, metric, NULL, per_id, per_distance);
    }
    if (rc) {
        free(per_distance);
        free(per_id);
        return rc;
    }
    if (prewhere)
        for (int i = 0; i < k * nq; i++)
            if (per_id[i] > -1) per_id[i] = (int64_t)actual_id_in_range[per_id[i]];

    float *out_d = (float *)malloc(sizeof(float) * k * nq);
    int64_t *out_i = (int64_t *)malloc(sizeof(int64_t) * k * nq);
    for (int q = 0; q < nq; q++) {
        size_t j = (size_t)q * k, z = (size_t)q * k, o = (size_t)q * k;
        for (int i = 0; i < k; i++, o++) {
            if ((metric != METRIC_IP && final_distance[j] > per_distance[z])
                || (metric == METRIC_IP && final_distance[j] < per_distance[z])) {
                out_d[o] = per_distance[z];
                out_i[o] = per_id[z] + num_rows_read;
                z++;
            } else {
                out_d[o] = final_distance[j];
                out_i[o] = final_id[j];
                j++;
            }
        }
    }
    memcpy(final_distance, out_d, sizeof(float) * k * nq);
    memcpy(final_id, out_i, sizeof(int64_t) * k * nq);
    free(out_d);
    free(out_i);
    free(per_distance);
    free(per_id);
    return 0;
}

/*
 * MergeTreeBaseSearchManager::getTotalTopSearchResultImpl
 * (src/VectorIndex/Storages/MergeTreeBaseSearchManager.cpp:207-299): cross-part top-k.
 * Every (score, part_index, label) goes into a std::multimap<Float32,...> in input
 * order (parts in order, ranks in order); asc: first k in map order (equal keys keep
 * insertion order); desc: reverse iteration (equal keys come out in REVERSE insertion
 * order).  Emulated with a stable sort.  Returns the number of results written.
 */
typedef struct {
    float score;
    uint64_t part;
    uint64_t label;
    size_t seq;
} mm_entry_t;

static int mm_cmp(const void *a, const void *b)
{
    const mm_entry_t *x = (const mm_entry_t *)a, *y = (const mm_entry_t *)b;
    if (x->score < y->score) return -1;
    if (x->score > y->score) return 1;
    return x->seq < y->seq ? -1 : (x->seq > y->seq ? 1 : 0);
}

ORACLE_API size_t oracle_total_topk(const float *scores, const uint64_t *parts, const uint64_t *labels, size_t n,
                                    size_t top_k, int desc, float *out_scores, uint64_t *out_parts,
                                    uint64_t *out_labels)
{
    mm_entry_t *e = (mm_entry_t *)malloc(sizeof(mm_entry_t) * (n ? n : 1));
    for (size_t i = 0; i < n; i++) {
        e[i].score = scores[i];
        e[i].part = parts[i];
        e[i].label = labels[i];
        e[i].seq = i;
    }
    qsort(e, n, sizeof(mm_entry_t), mm_cmp);
    size_t cnt = 0;
    for (size_t i = 0; i < n && cnt < top_k; i++, cnt++) {
        const mm_entry_t *s = desc ? &e[n - 1 - i] : &e[i];
        out_scores[cnt] = s->score;
        out_parts[cnt] = s->part;
        out_labels[cnt] = s->label;
    }
    free(e);
    return cnt;
}

/* ------------------------------------------------------------------ IVFFLAT */

/*
 * IVFFLAT search over a GIVEN index structure (centroids + list-major storage):
 * public Faiss IndexIVFFlat semantics behind Search::VectorIndex::search
 * (call site src/VectorIndex/Common/VIWithDataPart.cpp:922-926):
 *   1. coarse quantiser: exact k-NN (k = nprobe) of the query against the nlist
 *      centroids with the index metric (L2 or IP),
 *   2. scan the probed inverted lists exhaustively, 3. top-k.
 * Cosine indexes store L2-normalised rows; the caller normalises the query and
 * converts with 1 - ip (oracle_index_search below).
 * list_off[nlist+1] delimits list l as rows [list_off[l], list_off[l+1]) of vecs/ids.
 * alive (nullable) is indexed by ID (row offset in the part), like the reference's
 * filter bitmap (MergeTreeVSManager.cpp:434-438).
 */
ORACLE_API int oracle_ivf_search(const float *centroids, size_t nlist, const int64_t *list_off, const float *vecs,
                                 const int64_t *ids, const float *queries, size_t nq, size_t d, size_t nprobe,
                                 size_t k, int metric, const uint64_t *alive, int64_t *out_ids, float *out_dis,
                                 int64_t *out_probes /* nullable nq*nprobe */)
{
    if (metric != METRIC_L2 && metric != METRIC_IP) return 2;
    if (nprobe > nlist) nprobe = nlist;
    int64_t *pl = (int64_t *)malloc(sizeof(int64_t) * nprobe);
    float *pd = (float *)malloc(sizeof(float) * nprobe);
    cand_t *h = (cand_t *)malloc(sizeof(cand_t) * (k ? k : 1));
    for (size_t q = 0; q < nq; q++) {
        const float *xq = queries + q * d;
        oracle_knn(xq, centroids, d, nprobe, 1, nlist, metric, NULL, NULL, pl, pd);
        size_t cnt = 0;
        for (size_t p = 0; p < nprobe; p++) {
            if (out_probes) out_probes[q * nprobe + p] = pl[p];
            if (pl[p] < 0) continue;
            for (int64_t r = list_off[pl[p]]; r < list_off[pl[p] + 1]; r++) {
                if (alive && !bit_alive(alive, (size_t)ids[r])) continue;
                float v = metric == METRIC_IP ? oracle_ip(xq, vecs + r * d, d) : oracle_l2sqr(xq, vecs + r * d, d);
                topk_push(metric, h, k, &cnt, v, ids[r]);
            }
        }
        for (size_t j = 0; j < k; j++) {
            out_ids[q * k + j] = j < cnt ? h[j].id : -1;
            out_dis[q * k + j] = j < cnt ? h[j].dis : neutral(metric);
        }
    }
    free(pl);
    free(pd);
    free(h);
    return 0;
}

/* Plain Lloyd k-means for SMALL tests only (structure of a trained IVF index is
 * "parity unpinned"); deterministic: centroids start as the first
 * nlist points of a stride sample; empty clusters keep their previous centroid. */
ORACLE_API void oracle_kmeans(const float *x, size_t n, size_t d, size_t nlist, int iters, float *centroids)
{
    size_t stride = n / nlist ? n / nlist : 1;
    for (size_t c = 0; c < nlist; c++) memcpy(centroids + c * d, x + ((c * stride) % n) * d, sizeof(float) * d);
    double *sum = (double *)malloc(sizeof(double) * nlist * d);
    size_t *cnt = (size_t *)malloc(sizeof(size_t) * nlist);
    for (int it = 0; it < iters; it++) {
        memset(sum, 0, sizeof(double) * nlist * d);
        memset(cnt, 0, sizeof(size_t) * nlist);
        for (size_t i = 0; i < n; i++) {
            size_t best = 0;
            float bd = FLT_MAX;
            for (size_t c = 0; c < nlist; c++) {
                float v = oracle_l2sqr(x + i * d, centroids + c * d, d);
                if (v < bd) {
                    bd = v;
                    best = c;
                }
            }
            cnt[best]++;
            for (size_t j = 0; j < d; j++) sum[best * d + j] += x[i * d + j];
        }
        for (size_t c = 0; c < nlist; c++)
            if (cnt[c])
                for (size_t j = 0; j < d; j++) centroids[c * d + j] = (float)(sum[c * d + j] / (double)cnt[c]);
    }
    free(sum);
    free(cnt);
}

/* nearest-centroid assignment with canonical L2 (ties -> lowest centroid id) */
ORACLE_API void oracle_assign(const float *x, size_t n, size_t d, const float *centroids, size_t nlist,
                              int64_t *assign)
{
    for (size_t i = 0; i < n; i++) {
        size_t best = 0;
        float bd = FLT_MAX;
        for (size_t c = 0; c < nlist; c++) {
            float v = oracle_l2sqr(x + i * d, centroids + c * d, d);
            if (v < bd) {
                bd = v;
                best = c;
            }
        }
        assign[i] = (int64_t)best;
    }
}

/* ------------------------------------------------------------------ BM25 */

/*
 * Tantivy 0.21 BM25 (tantivy/src/query/bm25.rs, tantivy/src/fieldnorm/code.rs),
 * reached through TANTIVY::ffi_bm25_search (call sites
 * src/Storages/MergeTree/TantivyIndexStore.cpp:908-917,939-948):
 *   K1 = 1.2, B = 0.75
 *   idf(n, N)       = ln(1 + (N - n + 0.5) / (n + 0.5))                       (f32)
 *   norm(len_id)    = K1 * (1 - B + B * fieldnorm(len_id) / avg_fieldnorm)     (f32, 256-entry cache)
 *   score(term,doc) = idf * (1 + K1) * tf / (tf + norm(len_id(doc)))           (f32)
 *   avg_fieldnorm   = total_num_tokens / total_num_docs                        (f32 / f32)
 * with TABLE-LEVEL statistics (N, total tokens, df) passed in by the host
 * (ReadWithHybridSearch.cpp:89-209).  A multi-term OR query sums the term scores in
 * query-term order.  Golden: 00040_mqvs_hybrid_search.reference (2.1646233, 1.9431154).
 * Field length is quantised to a 1-byte fieldnorm id (Lucene SmallFloat byte4 scheme,
 * exact below 40 tokens).
 */
static uint32_t fieldnorm_table[256];
static int fieldnorm_table_ready = 0;

static void init_fieldnorm_table(void)
{
    if (fieldnorm_table_ready) return;
    for (uint32_t b = 0; b < 256; b++) {
        if (b < 24) {
            fieldnorm_table[b] = b;
        } else {
            uint32_t i = b - 24;
            uint32_t bits = i & 7;
            int shift = (int)(i >> 3) - 1;
            uint64_t dec = shift < 0 ? bits : ((uint64_t)(bits | 8) << shift);
            uint64_t v = 24 + dec;
            fieldnorm_table[b] = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v;
        }
    }
    fieldnorm_table_ready = 1;
}

ORACLE_API uint32_t oracle_fieldnorm_of_id(uint8_t id)
{
    init_fieldnorm_table();
    return fieldnorm_table[id];
}

/* largest id whose table value is <= len (tantivy fieldnorm_to_id) */
ORACLE_API uint8_t oracle_fieldnorm_id(uint32_t len)
{
    init_fieldnorm_table();
    int lo = 0, hi = 255;
    while (lo < hi) {
        int mid = (lo + hi + 1) / 2;
        if (fieldnorm_table[mid] <= len)
            lo = mid;
        else
            hi = mid - 1;
    }
    return (uint8_t)lo;
}

ORACLE_API float oracle_bm25_idf(uint64_t doc_freq, uint64_t doc_count)
{
    float x = ((float)(doc_count - doc_freq) + 0.5f) / ((float)doc_freq + 0.5f);
    return logf(1.0f + x);
}

/*
 * Postings in CSR form: term t owns postings [post_off[t], post_off[t+1]) of
 * (doc_ids, tfs); fieldnorm_ids[doc] is the quantised field length of each doc.
 * qterms[nq_terms] are the query's term indexes, df[nq_terms] the TABLE-level doc
 * frequencies, total_docs / total_tokens the table-level statistics.
 * Result: top-k by score descending, ties by ascending doc id (canonical).
 */
ORACLE_API size_t oracle_bm25_search(const int64_t *post_off, const uint32_t *doc_ids, const uint32_t *tfs,
                                     const uint8_t *fieldnorm_ids, size_t num_docs, const uint32_t *qterms,
                                     const uint64_t *df, size_t nq_terms, uint64_t total_docs, uint64_t total_tokens,
                                     const uint64_t *alive, size_t k, uint64_t *out_rows, float *out_scores)
{
    init_fieldnorm_table();
    const float K1 = 1.2f, B = 0.75f;
    float avg = (float)total_tokens / (float)total_docs;
    float cache[256];
    for (int i = 0; i < 256; i++) cache[i] = K1 * (1.0f - B + B * (float)fieldnorm_table[i] / avg);
    float *score = (float *)calloc(num_docs ? num_docs : 1, sizeof(float));
    uint8_t *hit = (uint8_t *)calloc(num_docs ? num_docs : 1, 1);
    for (size_t t = 0; t < nq_terms; t++) {
        float weight = oracle_bm25_idf(df[t], total_docs) * (1.0f + K1);
        for (int64_t p = post_off[qterms[t]]; p < post_off[qterms[t] + 1]; p++) {
            uint32_t doc = doc_ids[p];
            float tf = (float)tfs[p];
            float s = weight * (tf / (tf + cache[fieldnorm_ids[doc]]));
            score[doc] = score[doc] + s;
            hit[doc] = 1;
        }
    }
    cand_t *h = (cand_t *)malloc(sizeof(cand_t) * (k ? k : 1));
    size_t cnt = 0;
    for (size_t doc = 0; doc < num_docs; doc++)
        if (hit[doc] && bit_alive(alive, doc)) topk_push(METRIC_IP, h, k, &cnt, score[doc], (int64_t)doc);
    for (size_t j = 0; j < cnt; j++) {
        out_rows[j] = (uint64_t)h[j].id;
        out_scores[j] = h[j].dis;
    }
    free(h);
    free(score);
    free(hit);
    return cnt;
}

/*
 * The same scorer with several text columns and the AND operator (TantivyIndexStore.cpp:900-954 passes
 * `operator_or`; an fts index over several columns searches a token in every column).  Every (field, token) pair is a
 * term of its own: term_field[t] = its field (NULL: all field 0), fieldnorm_ids is [num_fields][num_docs],
 * total_tokens[num_fields]; df[j] is the TABLE-level document frequency of flat query term j, qgroups[j] the index of
 * the query token it stands for (NULL: j).  operator_or = 0 keeps the documents in which EVERY token group matched
 * (tantivy's conjunction of per-field disjunctions).  Scores sum in flat-term order.  PARITY UNPINNED for the
 * multi-field / AND cases: the reference's tests hold no golden for them (00040 / 00041 are single-column OR).
 */
ORACLE_API size_t oracle_bm25_search_ex(const int64_t *post_off, const uint8_t *term_field, const uint32_t *doc_ids,
                                        const uint32_t *tfs, const uint8_t *fieldnorm_ids, size_t num_fields,
                                        size_t num_docs, const uint32_t *qterms, const uint32_t *qgroups,
                                        const uint64_t *df, size_t nq_terms, uint64_t total_docs,
                                        const uint64_t *total_tokens, int operator_or, const uint64_t *alive, size_t k,
                                        uint64_t *out_rows, float *out_scores)
{
    init_fieldnorm_table();
    const float K1 = 1.2f, B = 0.75f;
    float *cache = (float *)malloc(sizeof(float) * 256 * num_fields);
    for (size_t f = 0; f < num_fields; f++) {
        float avg = (float)total_tokens[f] / (float)total_docs;
        for (int i = 0; i < 256; i++) cache[f * 256 + i] = K1 * (1.0f - B + B * (float)fieldnorm_table[i] / avg);
    }
    float *score = (float *)calloc(num_docs ? num_docs : 1, sizeof(float));
    uint32_t *hit = (uint32_t *)calloc(num_docs ? num_docs : 1, sizeof(uint32_t));
    uint32_t full = 0;
    for (size_t t = 0; t < nq_terms; t++) {
        uint32_t g = (qgroups ? qgroups[t] : (uint32_t)t) % 16;
        size_t f = term_field ? term_field[qterms[t]] : 0;
        full |= 1u << g;
        float weight = oracle_bm25_idf(df[t], total_docs) * (1.0f + K1);
        for (int64_t p = post_off[qterms[t]]; p < post_off[qterms[t] + 1]; p++) {
            uint32_t doc = doc_ids[p];
            float tf = (float)tfs[p];
            float s = weight * (tf / (tf + cache[f * 256 + fieldnorm_ids[f * num_docs + doc]]));
            score[doc] = score[doc] + s;
            hit[doc] |= 1u << g;
        }
    }
    cand_t *h = (cand_t *)malloc(sizeof(cand_t) * (k ? k : 1));
    size_t cnt = 0;
    for (size_t doc = 0; doc < num_docs; doc++)
        if (hit[doc] && (operator_or || hit[doc] == full) && bit_alive(alive, doc))
            topk_push(METRIC_IP, h, k, &cnt, score[doc], (int64_t)doc);
    for (size_t j = 0; j < cnt; j++) {
        out_rows[j] = (uint64_t)h[j].id;
        out_scores[j] = h[j].dis;
    }
    free(h);
    free(score);
    free(hit);
    free(cache);
    return cnt;
}

/* ------------------------------------------------------------------ fusion */

/*
 * Hybrid fusion (src/VectorIndex/Utils/HybridSearchUtils.cpp:164-314 and
 * MergeTreeHybridSearchManager::hybridSearch, MergeTreeHybridSearchManager.cpp:108-171).
 * Entries are keyed by (shard, part, label) in a std::map (ascending key order); the
 * fused scores are then inserted into a multimap<Float32, ..., greater> in that key
 * order, so equal scores come out in ascending (shard, part, label) order; first topk.
 * fusion_type: 0 = RRF, 1 = RSF.
 */
typedef struct {
    uint32_t shard;
    uint64_t part, label;
    float score;
} fuse_t;

static int fuse_key_cmp(const void *a, const void *b)
{
    const fuse_t *x = (const fuse_t *)a, *y = (const fuse_t *)b;
    if (x->shard != y->shard) return x->shard < y->shard ? -1 : 1;
    if (x->part != y->part) return x->part < y->part ? -1 : 1;
    if (x->label != y->label) return x->label < y->label ? -1 : 1;
    return 0;
}

static fuse_t *fuse_find(fuse_t *m, size_t *n, uint32_t shard, uint64_t part, uint64_t label)
{
    for (size_t i = 0; i < *n; i++)
        if (m[i].shard == shard && m[i].part == part && m[i].label == label) return &m[i];
    m[*n].shard = shard;
    m[*n].part = part;
    m[*n].label = label;
    m[*n].score = 0.0f;
    return &m[(*n)++];
}

/* computeNormalizedScore, HybridSearchUtils.cpp:276-314 */
static void normalized(const float *s, size_t n, float *out)
{
    if (n == 0) return;
    float mn = s[n - 1], mx = s[0];
    if (mn == mx) {
        for (size_t i = 0; i < n; i++) out[i] = 1.0f;
        return;
    }
    if (mn > mx) {
        float t = mn;
        mn = mx;
        mx = t;
    }
    float scale = mx - mn;
    for (size_t i = 0; i < n; i++) out[i] = (s[i] - mn) / scale;
}

static int fuse_score_cmp(const void *a, const void *b)
{
    const fuse_t *x = (const fuse_t *)a, *y = (const fuse_t *)b;
    /* a NaN score (RSF: inf / inf) ranks behind every other score; NaN scores among themselves by key.  (The reference's
     * multimap<float, greater> is undefined there; this is the order every implementation of the project keeps.) */
    const int nx = x->score != x->score, ny = y->score != y->score;
    if (nx != ny) return nx ? 1 : -1;
    if (x->score > y->score) return -1;
    if (x->score < y->score) return 1;
    return fuse_key_cmp(a, b);
}

ORACLE_API size_t oracle_hybrid_fusion(int fusion_type, const float *vec_scores, const uint64_t *vec_parts,
                                       const uint64_t *vec_labels, size_t nvec, const float *txt_scores,
                                       const uint64_t *txt_parts, const uint64_t *txt_labels, size_t ntxt,
                                       uint64_t fusion_k, float fusion_weight, int vector_scan_direction, size_t topk,
                                       float *out_scores, uint64_t *out_parts, uint64_t *out_labels)
{
    fuse_t *m = (fuse_t *)malloc(sizeof(fuse_t) * (nvec + ntxt + 1));
    size_t n = 0;
    if (fusion_type == 1) {
        float *norm = (float *)malloc(sizeof(float) * (nvec + ntxt + 1));
        normalized(txt_scores, ntxt, norm);
        for (size_t i = 0; i < ntxt; i++) fuse_find(m, &n, 0, txt_parts[i], txt_labels[i])->score = norm[i] * fusion_weight;
        normalized(vec_scores, nvec, norm);
        for (size_t i = 0; i < nvec; i++) {
            float v = vector_scan_direction == -1 ? norm[i] * (1 - fusion_weight) : (1 - norm[i]) * (1 - fusion_weight);
            fuse_find(m, &n, 0, vec_parts[i], vec_labels[i])->score += v;
        }
        free(norm);
    } else {
        if (fusion_k == 0) fusion_k = 60;
        for (size_t i = 0; i < nvec; i++) fuse_find(m, &n, 0, vec_parts[i], vec_labels[i])->score += 1.0f / (fusion_k + i + 1);
        for (size_t i = 0; i < ntxt; i++) fuse_find(m, &n, 0, txt_parts[i], txt_labels[i])->score += 1.0f / (fusion_k + i + 1);
    }
    qsort(m, n, sizeof(fuse_t), fuse_score_cmp);
    size_t cnt = n < topk ? n : topk;
    for (size_t i = 0; i < cnt; i++) {
        out_scores[i] = m[i].score;
        out_parts[i] = m[i].part;
        out_labels[i] = m[i].label;
    }
    free(m);
    return cnt;
}

/* ------------------------------------------------------------------ CPU-baseline legs (bench.py cpu_baseline only) */

/* Same algorithm as oracle_ivf_search / oracle_knn, OpenMP-parallel over queries.
 * The inner 64-wide accumulator loops auto-vectorise (AVX2, lane-wise IEEE, no
 * reassociation, -ffp-contract=off) so results stay bit-identical to the scalar oracle. */
ORACLE_API int oracle_ivf_search_mt(const float *centroids, size_t nlist, const int64_t *list_off, const float *vecs,
                                    const int64_t *ids, const float *queries, size_t nq, size_t d, size_t nprobe,
                                    size_t k, int metric, int64_t *out_ids, float *out_dis, int threads)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long q = 0; q < (long)nq; q++) {
        int r = oracle_ivf_search(centroids, nlist, list_off, vecs, ids, queries + (size_t)q * d, 1, d, nprobe, k,
                                  metric, NULL, out_ids + (size_t)q * k, out_dis + (size_t)q * k, NULL);
        if (r) rc = r;
    }
    return rc;
}

ORACLE_API int oracle_knn_mt(const float *x, const float *y, size_t d, size_t k, size_t nx, size_t ny, int metric,
                             int64_t *ids, float *dis, int threads)
{
    int rc = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (long q = 0; q < (long)nx; q++) {
        int r = oracle_knn(x + (size_t)q * d, y, d, k, 1, ny, metric, NULL, NULL, ids + (size_t)q * k,
                           dis + (size_t)q * k);
        if (r) rc = r;
    }
    return rc;
}
