/*
 * msvs_host.h -- C-ABI of libmsvs_host.so: the HOST side of the hot path, i.e. the parts the reference keeps in
 * clickhouse-server C++ above the native-library boundary, rebuilt on top of
 * libmsvs.so.  The C++ classes live in myscaledb_amd/host/msvs_host.hpp with the reference's names; these C entry
 * points exist so that tests (ctypes) and other hosts can drive them.  Pure host code: no HIP calls here except
 * through libmsvs.so's C-ABI.
 */
#ifndef MSVS_HOST_H
#define MSVS_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "msvs.h" /* msvs_index_t */

#ifdef __cplusplus
extern "C" {
#endif

#define MSVS_HOST_API __attribute__((visibility("default")))

/* VIWithColumnInPart::searchWithoutIndex<FloatVector> (src/VectorIndex/Common/VIWithDataPart.h:341-382):
 * cosine => normalise query and base IN PLACE (device kernel), IP search, d = 1 - d.  metric: msvs_metric. */
MSVS_HOST_API int msvs_host_search_without_index(float * query, float * base, size_t dim, size_t k, size_t nq,
                                                 size_t nbase, int metric, int64_t * labels, float * distances);

/* MergeTreeVSManager::searchWrapper<FloatVector> (src/VectorIndex/Storages/MergeTreeVSManager.cpp:1537-1679):
 * one brute-force block merged into the running (final_id, final_distance)[nq*k].
 * row_exists: LSB-first bitmap over the block's rows (nullable when delete_id_num == 0);
 * actual_id_in_range: nullable unless prewhere != 0. */
MSVS_HOST_API int msvs_host_search_wrapper(int prewhere, float * query, float * base, size_t nbase, int k, int dim,
                                           int nq, int num_rows_read, int64_t * final_id, float * final_distance,
                                           const uint64_t * actual_id_in_range, int metric,
                                           const uint64_t * row_exists, int delete_id_num);

/* MergeTreeVSManager::vectorScanWithoutIndex<FloatVector> (MergeTreeVSManager.cpp:959-1535): brute-force scan of one
 * data part, mark by mark, straight from the ColumnArray(Float32) layout (offsets[i] = end of row i in `data`).
 * filter_bits / row_exists_bits: nullable LSB-first bitmaps over the part's rows.  Outputs are sized nq*k by the
 * caller; *n_out = number of result rows (slots with id > -1); out_query_ids only written when is_batch != 0. */
MSVS_HOST_API int msvs_host_vector_scan_without_index(const uint64_t * offsets, const float * data, size_t rows,
                                                      size_t dim, size_t index_granularity, const float * queries,
                                                      size_t nq, int k, int metric, int is_batch,
                                                      const uint64_t * filter_bits, const uint64_t * row_exists_bits,
                                                      uint32_t * out_labels, uint32_t * out_query_ids,
                                                      float * out_distances, size_t * n_out);

/* The same scan over RESIDENT blocks (include/msvs.h msvs_cache_t): marks are uploaded once per part
 * (key = part_key / mark index), later queries only send their vectors; filters and lightweight deletes travel as row
 * bitmaps over the resident block.  Results are identical to msvs_host_vector_scan_without_index. */
struct msvs_cache;
struct msvs_comm;
MSVS_HOST_API int msvs_host_vector_scan_resident(struct msvs_cache * cache, const char * part_key, const uint64_t * offsets,
                                                 const float * data, size_t rows, size_t dim, size_t index_granularity,
                                                 const float * queries, size_t nq, int k, int metric, int is_batch,
                                                 const uint64_t * filter_bits, const uint64_t * row_exists_bits,
                                                 uint32_t * out_labels, uint32_t * out_query_ids, float * out_distances,
                                                 size_t * n_out);

/* Join of mergeSearchResultImpl (MergeTreeBaseSearchManager.cpp:23-164): out_pos[r] = index of part_offsets[r] in
 * labels, or -1 when the read row is not among the part's search results. */
MSVS_HOST_API void msvs_host_merge_search_result(const uint64_t * part_offsets, size_t n_rows, const uint32_t * labels,
                                                 size_t n_labels, int64_t * out_pos);

/* MergeTreeBaseSearchManager::getTotalTopSearchResultImpl (MergeTreeBaseSearchManager.cpp:207-299): cross-part
 * top-k through a multimap keyed by score; returns the number of results. */
MSVS_HOST_API size_t msvs_host_total_topk(const float * scores, const uint64_t * part_index, const uint64_t * labels,
                                          size_t n, size_t top_k, int desc_direction, float * out_scores,
                                          uint64_t * out_part_index, uint64_t * out_labels);

/* MergeTreeHybridSearchManager::hybridSearch + RankFusion / RelativeScoreFusion
 * (MergeTreeHybridSearchManager.cpp:108-171, src/VectorIndex/Utils/HybridSearchUtils.cpp:164-314).
 * fusion_type: 0 = RRF, 1 = RSF.  Inputs are the already ordered (best first) vector and text result lists. */
MSVS_HOST_API size_t msvs_host_hybrid_search(int fusion_type, const float * vec_scores, const uint64_t * vec_parts,
                                             const uint64_t * vec_labels, size_t nvec, const float * txt_scores,
                                             const uint64_t * txt_parts, const uint64_t * txt_labels, size_t ntxt,
                                             uint64_t fusion_k, float fusion_weight, int vector_scan_direction,
                                             size_t topk, float * out_scores, uint64_t * out_parts,
                                             uint64_t * out_labels);

/* The same fusion for a batch of queries straight from the device searches' output arrays (one part): query q's vector rows are
 * vec_dis / vec_ids[q * kv ...] (an id < 0 ends the list, like the host's `> -1` unpack, MergeTreeVSManager.cpp:1110-1140), its text
 * rows txt_scores / txt_ids[q * kt ...]; out_scores / out_labels[q * topk ...], n_out[q] rows each (the slots past them are left
 * as they were).  Order: descending fused score, ties by ascending label.  A row whose fused score is NaN (RSF: inf / inf for a
 * +inf distance at the head of a finite list) ranks behind every row whose score is not NaN, NaN rows among themselves by ascending
 * label, and they count in n_out like any other row: the order of msvs_hybrid_fuse_device (include/msvs.h).  The map-based
 * msvs_host_hybrid_search above keeps the reference's multimap, whose order is undefined once a score is NaN. */
MSVS_HOST_API int msvs_host_hybrid_search_batch(int fusion_type, const float * vec_dis, const int64_t * vec_ids, size_t kv,
                                                const float * txt_scores, const int64_t * txt_ids, size_t kt, size_t nq,
                                                uint64_t fusion_k, float fusion_weight, int vector_scan_direction, size_t topk,
                                                float * out_scores, uint64_t * out_labels, uint32_t * n_out);

/* HybridSearchFusionTransform::generate (src/VectorIndex/Processors/HybridSearchFusionTransform.cpp:22-182): the fusion step of
 * a Distributed-table hybrid search on the initiator.  Rows = the merged shard results in pipeline order: distance rows
 * (score_type 0) first, then bm25 rows (score_type 1), each with (shard_num, part_index, part_offset).  At most num_candidates
 * rows of each kind take part.  Output: indices into the input rows + fused scores (every bm25 row in order, then the
 * distance rows not among them); returns their number (<= 2 * num_candidates).  fusion_type: 0 = RRF, 1 = RSF. */
MSVS_HOST_API size_t msvs_host_fusion_transform(int fusion_type, const float * score, const uint8_t * score_type,
                                                const uint32_t * shard_num, const uint64_t * part_index, const uint64_t * part_offset,
                                                size_t n_rows, uint64_t num_candidates, uint64_t fusion_k, float fusion_weight,
                                                int vector_scan_direction, uint64_t * out_rows, float * out_scores);

/* Canonical merge of per-shard top-k lists that share one id space (the multi-GPU exchange step when the merge is
 * done on the host): ids/dis [nparts][nq][k] -> [nq][k]; order (dist asc | desc for IP, id asc; distances compare as floats, so
 * -0 and +0 tie).  An entry counts when its id is >= 0 and its distance is strictly better than the neutral value (< FLT_MAX,
 * IP: > -FLT_MAX; never NaN), as in msvs_merge_topk; unfilled slots are id -1 at that value.  The lists may be in any order, and
 * ids keep all 64 bits (the device forms carry 32).  L2 or IP, anything else MSVS_ERR_NOT_IMPLEMENTED. */
MSVS_HOST_API int msvs_host_merge_topk(const int64_t * ids, const float * dis, size_t nparts, size_t nq, size_t k,
                                       int metric, int64_t * out_ids, float * out_dis);

/* MergeTreeVSManager::generateVectorDataset + getQueryVector / getFloatQueryVectorInBatch
 * (MergeTreeVSManager.cpp:59-181): the query column of distance() / batch_distance() -- Array(Float32 | Float64) or
 * Array(Array(...)) -- flattened to nq x dim f32 row-major (Float64 by static_cast<float>, i.e. round to nearest).
 * values: the inner column's data (float or double, is_float64), offsets: the outer ColumnArray offsets (end of query q
 * in `values`), NULL for a single query of `dim` values.  A query whose length is not `dim` is the reference's
 * LOGICAL_ERROR "Dimension is not equal" / "wrong dimension": returns MSVS_ERR_INVALID_ARGUMENT (msvs_last_error()). */
MSVS_HOST_API int msvs_host_generate_vector_dataset(const void * values, int is_float64, const uint64_t * offsets,
                                                    size_t nq, size_t dim, float * out);

/* BM25InfoInDataParts-style statistics reduction (src/VectorIndex/Common/BM25InfoInDataParts.cpp:40-93):
 * element-wise sums of per-part (total_docs, total_tokens, df[n_terms]) vectors laid out [nparts][2 + n_terms]. */
MSVS_HOST_API void msvs_host_sum_bm25_stats(const uint64_t * per_part, size_t nparts, size_t n_terms, uint64_t * out);
/* The same sum across the GPUs of a sharded table: this rank's (total_docs, total_tokens, df[n_terms]) in `stats` [2 + n_terms]
 * (already summed over its own parts) becomes the table-wide vector on every rank -- one msvs_comm_all_reduce_u64 on the
 * communicator of the vector searches.  What the initiator of a Distributed query does with the shards' ftsIndex rows
 * (StorageFtsIndex.cpp:150-213) before any shard scores a document. */
MSVS_HOST_API int msvs_host_all_reduce_bm25_stats(const struct msvs_comm * comm, uint64_t * stats, size_t n_terms, void * hip_stream);

/* ---------------------------------------------------------------------------------------------- seam B host side
 * A part's text index as the device scorer consumes it (myscaledb_amd/host/text_store.cpp): the search-side interface
 * of TantivyIndexStore (src/Storages/MergeTree/TantivyIndexStore.cpp:900-992) over a POSTINGS EXPORT instead of a
 * tantivy index directory.  Errors: status code + msvs_text_last_error() (the host rethrows
 * TANTIVY_SEARCH_INTERNAL_ERROR, TantivyIndexStore.cpp:919-923). */
typedef struct msvs_text_index msvs_text_index_t;
typedef struct { const char * term; uint32_t field_id; uint64_t doc_freq; } msvs_doc_freq_t;       /* TANTIVY::DocWithFreq */
typedef struct { uint32_t field_id; uint64_t field_total_tokens; } msvs_field_tokens_t;            /* TANTIVY::FieldTokenNums */
typedef struct                                                                                     /* TANTIVY::Statistics */
{
    const msvs_doc_freq_t * docs_freq;
    size_t n_docs_freq;
    const msvs_field_tokens_t * total_num_tokens;
    size_t n_fields;
    uint64_t total_num_docs;
} msvs_bm25_stats_t;

MSVS_HOST_API const char * msvs_text_last_error(void);
/* The exporter (stands where ffi_create_index_with_parameter / ffi_index_multi_column_docs / ffi_index_writer_commit
 * stand, TantivyIndexStore.cpp:654-769): rows arrive in row order (row_id = 0, 1, ...); column_names[i] / docs[i] are
 * the (column, text) pairs of the row, an Array(String) column contributing several pairs.  commit() freezes the flat
 * postings and uploads them; save() writes the export file ("MSVSPOST" v1, layout in text_store.cpp), load() reads and
 * VALIDATES one (MSVS_ERR_IO on anything malformed) and uploads it. */
MSVS_HOST_API int msvs_text_index_create(const char * const * column_names, size_t ncols, msvs_text_index_t ** out);
MSVS_HOST_API void msvs_text_index_free(msvs_text_index_t * ix);
MSVS_HOST_API int msvs_text_index_add_doc(msvs_text_index_t * ix, uint64_t row_id, const char * const * column_names,
                                          const char * const * docs, size_t ncols);
MSVS_HOST_API int msvs_text_index_commit(msvs_text_index_t * ix);
MSVS_HOST_API int msvs_text_index_save(const msvs_text_index_t * ix, const char * path);
MSVS_HOST_API int msvs_text_index_load(const char * path, msvs_text_index_t ** out);
/* ffi_get_total_num_docs / ffi_get_total_num_tokens / ffi_get_doc_freq (TantivyIndexStore.cpp:957-992) */
MSVS_HOST_API uint64_t msvs_text_index_total_num_docs(const msvs_text_index_t * ix);
MSVS_HOST_API int msvs_text_index_total_num_tokens(const msvs_text_index_t * ix, msvs_field_tokens_t * out, size_t cap, size_t * n);
MSVS_HOST_API int msvs_text_index_doc_freq(const msvs_text_index_t * ix, const char * sentence, msvs_doc_freq_t * out, size_t cap,
                                           size_t * n);
/* The part's lightweight-delete bitmap in the reference's byte form (bit j of byte i = row 8 i + j,
 * MergeTreeTextSearchManager.cpp:199-255), kept resident on the device; NULL clears. */
/* Tokens of `text` under the default tokenizer chain (SimpleTokenizer on Unicode alphanumerics, RemoveLong(40), LowerCaser),
 * '\n'-separated; *n_needed = bytes incl. NUL (buf may be NULL / too small: call again). */
MSVS_HOST_API int msvs_text_tokenize(const char * text, char * buf, size_t cap, size_t * n_needed);
MSVS_HOST_API int msvs_text_index_set_alive(msvs_text_index_t * ix, const uint8_t * u8_alive_bitmap, size_t nbytes);
/* TANTIVY::ffi_bm25_search(index_path, sentence, column_names, topk, u8_alive_bitmap, use_filter, enable_nlq, operator_or,
 * statistics) (call sites TantivyIndexStore.cpp:908-917, 939-948) and its batched form.  Outputs [nq][topk], n_out[q] hits
 * each, best first.  enable_nlq != 0 -> MSVS_ERR_NOT_IMPLEMENTED. */
MSVS_HOST_API int msvs_text_index_bm25_search(const msvs_text_index_t * ix, const char * sentence, const char * const * column_names,
                                              size_t ncols, uint32_t topk, const uint8_t * u8_alive_bitmap, size_t nbytes,
                                              int use_filter, int enable_nlq, int operator_or, const msvs_bm25_stats_t * stats,
                                              uint64_t * row_ids, float * scores, uint32_t * n_out);
MSVS_HOST_API int msvs_text_index_bm25_search_batch(const msvs_text_index_t * ix, const char * const * sentences, size_t nq,
                                                    const char * const * column_names, size_t ncols, uint32_t topk,
                                                    const uint8_t * u8_alive_bitmap, size_t nbytes, int use_filter,
                                                    int enable_nlq, int operator_or, const msvs_bm25_stats_t * stats,
                                                    uint64_t * row_ids, float * scores, uint32_t * n_out);

/* Measurement / test driver for the reference's calling pattern (MergeTreeVSManager.cpp:973: up to ScanThreadLimiter-many host
 * threads, one query per VectorIndex::search call): `threads` native threads, thread t searching queries t, t + threads, ...
 * `calls_per_thread` times through msvs_index_search.  seconds: wall time; lat_us (nullable, [threads * calls_per_thread]):
 * per-call latencies; ids / dis (nullable, [n_queries][k]): each query's last result. */
MSVS_HOST_API int msvs_host_concurrent_search(const msvs_index_t * ix, const float * queries, size_t n_queries, size_t dim, int threads,
                                              size_t calls_per_thread, int k, const char * params, double * seconds, float * lat_us,
                                              int64_t * ids, float * dis);

/* Distributed BM25 statistics.  msvs_host_fts_index_statistics = the row ONE shard answers to
 * ftsIndex(db, table, column, query_text): total docs, per-field token totals and per-(term, field) document frequencies summed
 * over the shard's parts (ReadFromFtsIndex::initializePipeline, src/VectorIndex/Storages/StorageFtsIndex.cpp:150-213; a part
 * without a committed text index -> MSVS_ERR_NOT_IMPLEMENTED like the reference's missing index file).
 * msvs_host_fts_statistics_merge = the initiator's sum over the shards' rows (collectStatisticForBM25Calculation /
 * parseBM25StaisiticsInfo, src/VectorIndex/Utils/CommonUtils.cpp:190-330).  The view of either result is what the shards pass as
 * `stats` to msvs_text_index_bm25_search* (the "_fts_statistic_info" scalar); fields ordered by id, terms by (field_id, term). */
typedef struct msvs_fts_stats msvs_fts_stats_t;
MSVS_HOST_API int msvs_host_fts_index_statistics(const msvs_text_index_t * const * parts, size_t nparts, const char * query_text,
                                                 msvs_fts_stats_t ** out);
MSVS_HOST_API int msvs_host_fts_statistics_merge(const msvs_bm25_stats_t * const * rows, size_t nrows, msvs_fts_stats_t ** out);
MSVS_HOST_API const msvs_bm25_stats_t * msvs_fts_stats_view(const msvs_fts_stats_t * st);
MSVS_HOST_API void msvs_fts_stats_free(msvs_fts_stats_t * st);

#ifdef __cplusplus
}
#endif
#endif
