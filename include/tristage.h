/*
 * tristage.h — C ABI of the MI355X-native retrieval hot path of TriStage-RAG.
 *
 * This is the drop-in boundary.  The reference has no FFI of
 * its own: its native seam is the duck-typed FAISS index object held in
 * Stage1Retriever.faiss_index (reference src/stage1_retriever.py:126) plus
 * the per-candidate torch MaxSim in ColBERTScorer (src/stage2_rescorer.py:167-201).
 * Each entry point below names the reference call site it replaces.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative
 *     ts_status code, and ts_last_error() gives a thread-local message;
 *   - "device pointer" = HIP device memory on the index's device (e.g. a torch
 *     tensor's data_ptr()); `stream` is a hipStream_t passed as void* (NULL =
 *     the default stream);
 *   - the library owns the corpus memory after ts_index_add; the caller owns
 *     every output buffer; a handle is freed only by ts_index_destroy;
 *   - streams: every device-side step of a call (kernels, memsets, copies) is issued on `stream`, reads its device
 *     inputs in stream order (they may be the output of work still pending on `stream`) and is ordered before
 *     whatever the caller enqueues on `stream` afterwards.  The one use of the null stream is the zeroing of a
 *     workspace that has just been allocated (ts_index_create, ts_ivf_create, ts_ivf_reset, ts_bm25_set_index, a
 *     BM25 batch that needs more lanes than the handle has): the null stream is synchronised behind it before
 *     anything is enqueued on `stream`, which need not wait for the null stream.  Where an entry
 *     point's own comment does not say more: ts_index_add, ts_index_reconstruct, ts_index_range_fetch,
 *     ts_index_live_words, ts_index_compact, ts_index_remove and ts_index_update return after a synchronisation of
 *     `stream` behind their last step; so does every IVF call that takes a stream, ts_mmr_ivf excepted, and so do
 *     the ts_bm25_search calls, whose results are host memory.  The stateless calls ts_merge_topk(_strided),
 *     ts_maxsim, ts_maxsim_indexed(_batch)(_fp8), ts_quantize_rows_fp8 and the forward kernels only enqueue on
 *     `stream` and return without a host synchronisation; two cases wait for `stream` all the same: a MaxSim call
 *     whose scratch for that (device, stream) has to grow, and a merge of more than 16384 / k lists, which frees
 *     its intermediate lists before it returns.  ts_index_read_probe times its passes with events and waits for them.
 *   - threading: ts_index_search on a built index is safe for
 *     concurrent callers on ONE handle that use distinct streams and output
 *     buffers: each call takes one of 8 internal workspace sets (a 9th
 *     synchronous caller waits for a set), its own report slot, and the exact
 *     fallback of a synchronous call runs on that call's set.  Host-pointer
 *     searches (TS_FLAG_HOST_PTR) share one staging area and are serialised
 *     inside the handle, as are searches while per-phase profiling is on.
 *     Asynchronous submission (TS_FLAG_ASYNC + ts_index_finish) is for ONE
 *     submitting thread per handle at a time; synchronous searches from other
 *     threads may run beside it.  add / reset / reserve / set_id_offset /
 *     destroy need exclusive access.  The stateless entry points (ts_merge_topk*,
 *     ts_maxsim*, and the forward kernels ts_add_layernorm / ts_add_prenorm /
 *     ts_embed_layernorm / ts_attention_varlen / ts_rope_inplace / ts_geglu /
 *     ts_linear_*) are
 *     thread-safe; a ts_bm25 handle serves one caller at a time; per-kernel device attributes are set once per
 *     device under a lock, so one process may drive several GPUs.
 */
#ifndef TRISTAGE_H_
#define TRISTAGE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing signature or the meaning of an argument changes, or entry points are added
 * (a caller built against version N may load any library whose ts_abi_version() == N; nothing older, nothing
 * newer).  1 = round 1 (24 entry points).  2 = round 2 changed ts_attention_varlen (offsets, window, rotary
 * tables) and added 15 entry points.  3 = round 3 added ts_index_read_probe, ts_index_filter_path and
 * ts_linear_add_layernorm, ts_mlp_add_layernorm.  4 = filtered search: ts_index_search_filtered,
 * ts_index_last_filter_info and ts_bm25_search_batch_filtered (no existing signature changed).  Coalesced passes
 * (TS_FLAG_COALESCE, ts_index_flush, ts_coalesce_groups) were added within version 4: no signature changed, and a
 * caller that never sets the flag sees the library it was built against.  The IVF-Flat entry points (ts_ivf_*) were
 * added within version 4 as well: no existing signature changed.  So were wide coalesced passes
 * (TS_FLAG_WIDE_PASSES, TS_FLAG_NO_WIDE_PASSES, ts_coalesce_groups_wide, ts_coalesce_wide_min_bytes), query-stationary
 * passes (TS_FLAG_STATIONARY_PASSES, TS_FLAG_NO_STATIONARY_PASSES, ts_coalesce_groups_stationary), their pass
 * prologue (TS_FLAG_PASS_PROLOGUE, TS_FLAG_NO_PASS_PROLOGUE), and removal
 * (ts_index_remove, ts_index_live_count, ts_index_live_words, ts_index_compact): no existing signature changed, and
 * an index from which nothing is removed behaves as before; so was ts_remove_ivf.  So were ts_index_update and
 * ts_update_ivf: an index that is never updated runs the code it ran before.  So was ts_compact_ivf: no existing
 * signature changed, and an index that is never compacted runs the code it ran before.  So were ts_index_range_search
 * and ts_index_range_fetch: no existing signature changed, and a caller that never runs a range search sees the
 * library it was built against (no existing kernel changed).  So was e4m3 index storage (ts_index_create accepts
 * TS_FP8_E4M3; ts_index_set_fp8_scale_log2, ts_index_fp8_scale_log2): no existing signature changed, and an index of
 * another storage dtype runs the kernels it ran before.  So was 4-bit MX index storage (ts_index_create accepts
 * TS_MXFP4_E2M1): no signature changed. So were ts_index_mmr, ts_mmr_ivf and the measurement aid
 * ts_index_mmr_set_timing / ts_index_mmr_get_timings: no existing signature or kernel changed, and a caller that
 * never calls them allocates and launches nothing new.  So was ts_group_topk, on the same terms.  So were
 * ts_maxsim_passages_indexed and ts_maxsim_passages_indexed_batch, on the same terms.  So were ts_index_search_prefix
 * and ts_index_rescore, on the same terms.  So were ts_index_search_biased and ts_index_last_bias_info, on the same
 * terms.                                                                                                             */
#define TS_ABI_VERSION 4

typedef struct ts_index ts_index; /* opaque */

enum ts_status {
  TS_OK = 0,
  TS_ERR_INVALID = -1,   /* bad argument */
  TS_ERR_HIP = -2,       /* a HIP runtime call failed */
  TS_ERR_OOM = -3,       /* device allocation failed */
  TS_ERR_EMPTY = -4,     /* search on an index with no rows
                            (reference: ValueError "No documents indexed",
                            src/stage1_retriever.py:370-371) */
  TS_ERR_UNSUPPORTED = -5
};

enum ts_dtype { TS_F32 = 0, TS_F16 = 1, TS_BF16 = 2,
               TS_FP8_E4M3 = 3 /* OCP e4m3fn: a storage dtype of ts_index_create ("e4m3 index storage" below) and the
                                  element type of the e4m3 token-store entry points; never a rows / query dtype */,
               TS_MXFP4_E2M1 = 4 /* OCP e2m1 elements with one E8M0 scale per 32: a storage dtype of ts_index_create only
                                    ("4-bit MX index storage" below); never a rows / query / store dtype */ };

enum ts_metric { TS_METRIC_INNER_PRODUCT = 0 };

/* ts_index_add / ts_index_search flags */
#define TS_FLAG_HOST_PTR 1u     /* `rows` / `queries` / outputs are host memory */
#define TS_FLAG_NO_FILTER 2u    /* search: force the dense (materialise+select) path */
#define TS_FLAG_ASYNC 8u        /* search: enqueue only (device pointers); results are valid
                                   and verified after ts_index_finish()            */
#define TS_FLAG_PIPELINE 16u    /* with TS_FLAG_ASYNC: overlap this search's query preparation and
                                   final selection with the scans of its neighbours (internal
                                   streams).  The caller guarantees that `queries` is already
                                   complete in memory when the call is made (not the output of
                                   work still pending on `stream`); results are ordered after
                                   the call on `stream` as usual.                             */
#define TS_FLAG_CLASSIC 32u     /* search: take the five-launch filter path (query prep, sample scan,
                                   thresholds, scan+filter, select) even where the one-launch scan
                                   (query image, thresholds and scan+filter in ONE kernel) is the
                                   default: A/B measurements and tests; results are identical    */
#define TS_FLAG_ONE_LAUNCH 64u  /* search: take the one-launch scan wherever its threshold estimate is
                                   valid, also where the five-launch path is the default (pipelined
                                   submission, corpora above 4 M rows); results are identical      */
#define TS_FLAG_COALESCE 128u   /* with TS_FLAG_ASYNC: the search's filter scan may be held until other
                                   batches arrive, so that one corpus pass serves up to
                                   ts_coalesce_groups() 32-query groups (see "coalesced passes"
                                   below).  Results are identical; they are complete after
                                   ts_index_finish() (or ts_index_flush() and stream order).    */
#define TS_FLAG_WIDE_PASSES 256u     /* with TS_FLAG_COALESCE: wide passes (ts_coalesce_groups_wide() groups)
                                        whatever the corpus size; results are identical              */
#define TS_FLAG_NO_WIDE_PASSES 512u  /* with TS_FLAG_COALESCE: never wide passes (ts_coalesce_groups())  */
#define TS_FLAG_STATIONARY_PASSES 1024u     /* with TS_FLAG_COALESCE: query-stationary passes
                                               (ts_coalesce_groups_stationary() groups) wherever their kernel
                                               exists, whatever the corpus size; results are identical        */
#define TS_FLAG_NO_STATIONARY_PASSES 2048u  /* with TS_FLAG_COALESCE: never query-stationary passes          */
#define TS_FLAG_PASS_PROLOGUE 4096u     /* with TS_FLAG_COALESCE: in a queue of query-stationary passes of an index
                                           without removed rows, a batch's sample scan and thresholds are enqueued
                                           with its first pass, and a pass's sample scans, thresholds and selects
                                           share one launch each ("pass prologue"); the default there, and without
                                           effect elsewhere; results are identical                              */
#define TS_FLAG_NO_PASS_PROLOGUE 8192u  /* with TS_FLAG_COALESCE: never: every batch keeps launches of its own  */
#define TS_FLAG_NORMALIZE 4u    /* add: L2-normalise rows x/(|x|+1e-8) on device first
                                   (reference src/stage1_retriever.py:285-288) */

/* ---- index lifetime ------------------------------------------------------
 * replaces faiss.IndexFlatIP(d) (reference src/stage1_retriever.py:263,276).
 * storage_dtype: element type the corpus is kept in (TS_F32 = FAISS-exact
 * storage; TS_F16 / TS_BF16 halve the bytes scanned; TS_FP8_E4M3 halves them
 * again, see "e4m3 index storage" below; TS_MXFP4_E2M1 once more, see
 * "4-bit MX index storage").                                                 */
int ts_index_create(int32_t dim, int32_t storage_dtype, int32_t metric,
                    int32_t device, ts_index** out);
int ts_index_destroy(ts_index* h);
/* drop all rows, keep the allocation */
int ts_index_reset(ts_index* h);
/* pre-size the corpus allocation for `nrows` rows in total */
int ts_index_reserve(ts_index* h, int64_t nrows);

/* ---- add -----------------------------------------------------------------
 * replaces faiss_index.add(float32[n,d]) (src/stage1_retriever.py:270,277,313).
 * rows: row-major [n, dim] of rows_dtype (device pointer unless
 * TS_FLAG_HOST_PTR).  Rows are appended; ids are assigned consecutively.    */
int ts_index_add(ts_index* h, const void* rows, int64_t n, int32_t rows_dtype,
                 uint32_t flags, void* stream);

/* ---- search --------------------------------------------------------------
 * replaces faiss_index.search(float32[B,d], k) (src/stage1_retriever.py:380):
 * exact inner product of each query against every row; out_scores[B,k]
 * sorted descending, ties by ascending id; out_ids[B,k] int64; when k exceeds
 * the row count the tail is padded with id -1 / score -FLT_MAX (FAISS's
 * convention, which the reference filters at src/stage1_retriever.py:383).
 * Ids are row numbers plus the offset set by ts_index_set_id_offset.
 * The order in full ("selection order"): score descending with
 * -0 equal to +0 (a zero comes back as +0); a NaN of either sign ranks below
 * -inf; exactly equal scores by ascending id, whatever the size of the tie.
 * Synchronous with respect to `stream` on return.                            */
int ts_index_search(ts_index* h, const void* queries, int32_t nq,
                    int32_t q_dtype, int32_t k, float* out_scores,
                    int64_t* out_ids, uint32_t flags, void* stream);

/* ---- filtered search -------------------------------------------------------
 * ts_index_search restricted per query to an allowed set of rows: the result is exactly what
 * ts_index_search would return on an index holding only the allowed rows, with their original ids
 * (scores descending, ties by ascending id, padded with id -1 / -FLT_MAX when a query has fewer than k
 * allowed rows), and every allowed row's score is bit-identical to its score in an unfiltered search.
 *   allow_bits     n_masks masks of allow_words uint32 words each (device memory; host memory with
 *                  TS_FLAG_HOST_PTR).  Bit r % 32 of word r / 32 set = local row r allowed (local rows
 *                  are numbered before ts_index_set_id_offset).  Bits at or beyond ntotal are ignored;
 *                  allow_words >= ceil(ntotal / 32).
 *   mask_of_query  HOST array of nq entries in [-1, n_masks); -1 = the query is not filtered.  Queries of
 *                  one pass may share a mask.
 * Flags as for ts_index_search: TS_FLAG_HOST_PTR, TS_FLAG_NO_FILTER, TS_FLAG_ASYNC (the masks are read in
 * stream order; ts_index_finish verifies the search and reports it for a redo like any other).
 * TS_FLAG_PIPELINE and TS_FLAG_ONE_LAUNCH are ignored for passes with a mask: they take the five-launch
 * path (the one-launch kernel has no masked form).  Per pass of <= 64 queries the GPU builds the list of
 * row blocks (32 rows) whose OR over the pass's masks is non-zero, and the scan reads only those.  fp32
 * storage takes the exact dense path with the masks applied at selection.  Invalid arguments return
 * TS_ERR_INVALID before any HIP call.                                                                   */
int ts_index_search_filtered(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k,
                             const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                             const int32_t* mask_of_query, float* out_scores, int64_t* out_ids,
                             uint32_t flags, void* stream);
/* the last ts_index_search_filtered call on this handle, summed over its passes that had a mask:
 * [0] row blocks the scans read (live blocks; a pass on the dense path reads them all), [1] row blocks
 * of the index, [2] passes on the masked filter path, [3] passes on the dense path.  For an asynchronous
 * call [0] is complete after ts_index_finish.  The redo of a ticket that ts_index_finish reports is a new
 * ts_index_search_filtered call: read the counters of the submitted searches before it.                */
int ts_index_last_filter_info(const ts_index* h, int64_t info[4]);

/* ---- range search ----------------------------------------------------------
 * FAISS range_search: for query q with radius[q] (a float32 on the index's score scale) every live row with
 * score(q, row) >= radius[q]; with masks, only the allowed rows count.  Added within version 4.
 *   - The bound is inclusive; the comparison is the float >= of the filter scan.  A NaN score is never returned.
 *     A NaN radius is TS_ERR_INVALID before any HIP call.  -inf returns every live (allowed) row.
 *   - Scores are bit-identical to those of ts_index_search / ts_index_scores on the same rows (same query image,
 *     same MFMA k-group order).
 *   - The result is in FAISS's CSR form: lims (HOST int64[nq + 1]); query q owns entries [lims[q], lims[q + 1]) of
 *     the packed scores and ids.  WITHIN A QUERY THE ROWS ARE IN ASCENDING ID ORDER, on every path (FAISS promises
 *     no order).  Ids carry the id offset.  Removed rows are never returned; after ts_index_compact the ids are the
 *     new ones.
 *   - Every storage type, any nq (passes of <= 64 queries), tombstones, and masks with the semantics of
 *     ts_index_search_filtered (allow_bits / allow_words / n_masks / mask_of_query as there, ANDed with the live
 *     set); mask_of_query may be NULL: unfiltered.  radius is a HOST array of nq floats.
 *   - Synchronous only; held coalesced passes are flushed first.  Flags: TS_FLAG_HOST_PTR (queries and masks are host
 *     memory), TS_FLAG_NO_FILTER (force the dense path: tests, A/B runs).
 *   - max_total bounds the number of entries of the call (<= 0: 1 << 26 entries, 12 bytes each).  Every pass's total
 *     is known on the host before anything of it is written; if the running total would pass the limit the call
 *     returns TS_ERR_UNSUPPORTED, lims hold the counts so far (flat behind them), ts_last_error() names the total and
 *     the limit, nothing is stored and the index stays usable.
 * Per pass: the query image; then, from 32768 rows, the filter scan of ts_index_search with the radii as its
 * thresholds (its masked form with masks or tombstones), whose per-query counts are exact also past its 16384
 * candidate slots; if no count exceeds them, one workgroup per query sorts its (id, score) pairs by id.  Otherwise,
 * and for smaller corpora and fp32 storage with masks or tombstones, the whole pass takes the dense path: dense scores
 * in chunks of 2^20 rows, counted per 1024-row tile, prefixed, and written in place by rank.
 * The packed result stays in the handle: ts_index_range_fetch copies the lims[nq] entries of the last range search to
 * out_scores (float) / out_ids (int64), device memory or host memory with TS_FLAG_HOST_PTR; a capacity (entries) that
 * is too small is TS_ERR_INVALID.  The stored result is valid until the next range search, add, remove, update,
 * compact, reset or destroy on the handle.  ts_index_last_search_info after a range call: [0] 32 + (0 every pass
 * dense, 1 filter scans, 2 a filter pass was redone densely), [1] passes, [2] passes that ran the filter scan,
 * [3] those of them that were redone densely.                                                                    */
int ts_index_range_search(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, const float* radius,
                          const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                          const int32_t* mask_of_query, int64_t max_total, int64_t* lims, uint32_t flags,
                          void* stream);
int ts_index_range_fetch(ts_index* h, float* out_scores, int64_t* out_ids, int64_t capacity, uint32_t flags,
                         void* stream);

/* ---- all scores, no selection -----------------------------------------------
 * replaces the numpy product in EmbeddingService.similarity (reference
 * src/embedding_service.py:228-237: cosine of one query against a document
 * matrix, result in document order): out[q*ld + row] = <query q, row> for every
 * row; ld is a multiple of 4 and >= ntotal rounded up to 32 (the entries
 * [ntotal, that bound) of each line are set to -FLT_MAX), `out` device memory,
 * 16-byte aligned.  Synchronous with respect to `stream` on return.            */
int ts_index_scores(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype,
                    float* out, int64_t ld, void* stream);

/* ---- asynchronous searches ------------------------------------------------
 * With TS_FLAG_ASYNC ts_index_search only enqueues work on `stream` and returns;
 * consecutive batches then run back to back on the GPU with no host round trip
 * in between.  Each call gets a ticket (ts_index_last_ticket).  ts_index_finish
 * synchronises the stream once and checks every unfinished search: the tickets
 * whose fused filter could not prove exactness (rare) are
 * returned in failed_tickets[0..*n_failed) and must be repeated by the caller
 * with TS_FLAG_NO_FILTER (synchronously).  At most 256 passes (of <= 64 queries each; <= 32 where the query
 * image of 64 does not fit LDS) may be unfinished (round 2: 64 — a collective finish every 30 batches cost the
 * sharded path 4-7 % of its time at 2.5 M / 1.25 M rows per rank).                                              */
int64_t ts_index_last_ticket(const ts_index* h);
/* 1 if a search for top-k on this index takes the threshold-filter path (exact only once verified: a synchronous
 * call verifies before it returns, an asynchronous one in ts_index_finish), 0 if it takes the dense path, whose result
 * is exact by construction — an asynchronous search is then final when the stream reaches it, so a caller may consume
 * it in stream order without waiting (the per-query path of RetrievalPipeline.search on small corpora: no host sync
 * between faiss_index.search, reference src/stage1_retriever.py:380, and stage 2).  Negative: error.          */
int ts_index_filter_path(const ts_index* h, int32_t k);
int ts_index_finish(ts_index* h, void* stream, int64_t* failed_tickets, int32_t max_failed,
                    int32_t* n_failed);

/* ---- coalesced passes (TS_FLAG_COALESCE | TS_FLAG_ASYNC) ------------------------
 * An unfiltered, unpipelined asynchronous search on the five-launch filter path (corpora above 4 M rows, or
 * TS_FLAG_CLASSIC) enqueues its query preparation, sample scan and thresholds on `stream` at once (the queries
 * are read in stream order, as without the flag) and puts its 32-query groups in a pending-pass queue on the
 * handle.  When the queue holds ts_coalesce_groups() groups, one filter scan over the corpus serves them all,
 * and the select of every batch whose last group was in it follows on the same stream.  Groups of different
 * batches, sizes and k share a pass; a batch of 64 may straddle two passes.  A search that cannot join
 * (other flags, a filtered search, another stream, the one-launch or dense path, fewer than 3 groups per pass)
 * joins nothing and is ordered behind the held work.  The queue is flushed — a partial pass is launched — by
 * ts_index_finish, ts_index_flush, any search that cannot join, ts_index_add / reset / reserve /
 * set_id_offset / reconstruct / scores / destroy (a held batch searches the corpus it was submitted against),
 * and the unfinished-pass limit.  Tickets, verification and redo are those of any asynchronous search.
 * Not for callers that consume results in stream order before ts_index_finish without ts_index_flush.       */
/* enqueue every held pass on the queue's stream; `stream`'s later work is ordered behind it.  No host sync. */
int ts_index_flush(ts_index* h, void* stream);
/* 32-query groups per coalesced pass for this dimension and storage type: 4 up to a padded dimension of 512,
 * 3 at 640 and 768, 2 from 896 (no coalescing below 3), 0 for fp32 storage.  Needs no GPU.                   */
int32_t ts_coalesce_groups(int32_t dim, int32_t storage_dtype);
/* Wide passes: LDS holds a double-buffered window of the groups' query images instead of the whole images, so a
 * pass takes ts_coalesce_groups_wide() groups at any dimension (6 for f16 / bf16 storage, 0 for fp32).  The queue
 * uses them where the corpus (rows rounded up to 32 x padded dimension x element size) is larger than
 * ts_coalesce_wide_min_bytes() and ts_coalesce_groups() is at most 3 (a padded dimension above 512), unless
 * TS_FLAG_WIDE_PASSES / TS_FLAG_NO_WIDE_PASSES decide.  A queue holds groups
 * of one width: a search that asks for the other flushes it first.  Added within version 4.  Need no GPU.     */
int32_t ts_coalesce_groups_wide(int32_t dim, int32_t storage_dtype);
int64_t ts_coalesce_wide_min_bytes(void);
/* Query-stationary passes: each of a workgroup's eight waves keeps one group's query image in registers and the
 * corpus goes through LDS once per compute unit, so a pass takes ts_coalesce_groups_stationary() groups: 8 for
 * f16 / bf16 storage at a padded dimension of 640 or 768 (512 < dim <= 768), 0 otherwise (the image of a larger
 * dimension does not fit the registers; at a smaller one the LDS-resident passes read at the ceiling already).  The
 * queue uses them where it would use wide passes by its own policy (neither wide-pass flag set) and nothing has been
 * removed from the index, unless TS_FLAG_STATIONARY_PASSES / TS_FLAG_NO_STATIONARY_PASSES decide; a forced
 * TS_FLAG_WIDE_PASSES / TS_FLAG_NO_WIDE_PASSES keeps the widths it had.  Added within version 4.  Needs no GPU.
 * Pass prologue: in a queue of these passes, while nothing is removed, only the query preparation of a batch is
 * enqueued when it is submitted (it alone reads the caller's queries); its sample scan and thresholds are enqueued in
 * front of the first pass that holds one of its groups, and a pass's sample scans, thresholds and selects share one
 * launch each.  TS_FLAG_NO_PASS_PROLOGUE keeps every batch's own launches; a queue holds one setting, and a search
 * that asks for the other flushes it first.  Results, reports and redo are the same.  Added within version 4.       */
int32_t ts_coalesce_groups_stationary(int32_t dim, int32_t storage_dtype);

/* ---- removal (tombstones) ------------------------------------------------
 * FAISS remove_ids with stable ids: a removed row keeps its id, is never returned by a search, and keeps its
 * storage until ts_index_compact.  ntotal keeps counting every id ever assigned; rows added later get ids from
 * ntotal upward.  While nothing is removed no search reads the tombstones.  After a removal every search is the
 * filtered search (ts_index_search_filtered) of the live rows: ts_index_search equals ts_index_search_filtered with
 * the live set as its mask, bit for bit, and a filtered search's masks are ANDed with the live set.  Added within
 * version 4.  Exclusive access, as add.
 *   remove       ids (HOST int64[n]) as search returns them, i.e. after the id offset; unknown, repeated and
 *                already removed ids are skipped and not counted (*n_removed).  Held coalesced passes are flushed
 *                first and the update is ordered on `stream` behind every search submitted before it, so those
 *                see the index as it was.  A search that ts_index_finish reports for a redo is redone against
 *                the index as it is then: finish before removing where that matters.
 *   live_count   rows not removed.
 *   live_words   the live set, HOST uint32[ceil(ntotal / 32)]: bit r % 32 of word r / 32 = row r live.
 *   compact      moves the live rows down in place (order kept; ts_index_scores / reconstruct see the new rows),
 *                ntotal = live_count afterwards; old2new (HOST int64[old ntotal], -1 = removed; may be NULL)
 *                receives the monotone map.  On the device: a prefix count over the live words, then ascending
 *                chunks of whole row blocks gathered through a 256 MiB staging buffer and copied back.          */
int ts_index_remove(ts_index* h, const int64_t* ids, int64_t n, int64_t* n_removed, void* stream);
int64_t ts_index_live_count(const ts_index* h);
int ts_index_live_words(ts_index* h, uint32_t* out, void* stream);
int ts_index_compact(ts_index* h, int64_t* old2new, void* stream);

/* ---- update in place ------------------------------------------------------
 * Replaces stored rows and keeps their ids.  Reference call site: none; the reference never changes a stored vector
 * (its FAISS index is only ever added to, reference src/stage1_retriever.py:283).  Added within version 4.
 * Exclusive access, as add.
 *   ids      HOST int64[n], as search returns them, i.e. after the id offset.
 *   rows     [n, dim] of rows_dtype, row i replacing id ids[i]; DEVICE, or HOST with TS_FLAG_HOST_PTR.
 *   flags    TS_FLAG_NORMALIZE, TS_FLAG_HOST_PTR, as ts_index_add takes them.
 * Afterwards the index holds the bytes ts_index_add of the final matrix would have written: the rows go through
 * add's own relayout (rounding, normalisation), by one of two routes.  Ids that are one ascending run of consecutive
 * rows are relaid out straight into the corpus at those rows (the relayout writes the units of the rows it is given
 * and of no other); no staging, no further kernel.  Any other ids are relaid out into a staging tile, and 16-byte
 * units move from there to their places: a row block all of whose 32 rows are updated is written as whole 1 KiB unit
 * rows, of any other block only the updated rows' units are written.
 * All or nothing: an id outside [0, ntotal), an id given twice in the call, or the id of a removed row fails the
 * call with TS_ERR_INVALID, a message naming the first such id, and nothing written (ts_index_remove skips
 * unknown ids; a skipped update would lose data silently).
 * Ordering as ts_index_remove: held coalesced passes are flushed first and the update is ordered on `stream` behind
 * every search submitted before it, so those read the rows as they were.  The tombstones, ntotal, live_count and
 * the id offset do not change.                                                                                   */
int ts_index_update(ts_index* h, const int64_t* ids, int64_t n, const void* rows, int32_t rows_dtype,
                    uint32_t flags, void* stream);

/* ---- introspection -------------------------------------------------------
 * faiss_index.ntotal / .d                                                    */
int64_t ts_index_ntotal(const ts_index* h);
int32_t ts_index_dim(const ts_index* h);
int32_t ts_index_dtype(const ts_index* h);

/* ---- e4m3 index storage (TS_FP8_E4M3) ----------------------------------------------------------
 * One byte per element, scored in place.  An index carries one scale exponent s (0 .. 15, default 8): element x is
 * stored as e4m3fn_rne(x * 2^s): round to nearest even, e4m3 subnormals kept, |x * 2^s| > 448 and +-Inf saturate to
 * +-448, NaN stores 0x7F.  There is no per-row scale (scores are compared across rows), so add, update and several
 * adds are bit-reproducible; with TS_FLAG_NORMALIZE the f32 quotient x / (|x| + 1e-8) is quantised.  Unit-norm rows
 * fit the default (|x_i| <= 1 <= 448 / 256).  Queries are rounded to bf16 whatever their dtype; a score equals, bit
 * for bit, that of a TS_BF16 index holding the decoded rows.  ts_index_reconstruct returns the decoded values
 * e4m3 * 2^-s.  dim is padded to a multiple of 256 and is at most 2048.
 * Supported: add, reserve, reset, id offset, reconstruct, search (synchronous, asynchronous), search_filtered, scores,
 * remove, compact, update.  TS_FLAG_ONE_LAUNCH, TS_FLAG_PIPELINE, TS_FLAG_COALESCE and the wide-pass flags are ignored
 * (ts_coalesce_groups* return 0 for it); ts_index_range_search returns TS_ERR_UNSUPPORTED, and there is no IVF form.
 * ts_index_set_fp8_scale_log2: TS_ERR_INVALID for s outside 0 .. 15, for an index of another storage dtype, and once
 * the index holds rows (ts_index_reset empties it).  ts_index_fp8_scale_log2: s, or -1 for another storage dtype.  */
int ts_index_set_fp8_scale_log2(ts_index* h, int32_t s);
int32_t ts_index_fp8_scale_log2(const ts_index* h);
/* ---- diversified selection: maximal marginal relevance --------------------------------------
 * Reference call site: none (the reference returns the plain top-k of overlapping chunks, src/utils.py chunk_text).
 * Added within version 4: no existing signature or kernel changed, and a caller that never calls these allocates
 * and launches nothing new.
 * Per query: fetch_k candidate ids (cand_ids [nq, fetch_k] int64, in the id space search returns, i.e. with the id
 * offset; -1 = padding) with their relevances (cand_rel [nq, fetch_k] float32), and k picks, 1 <= k <= fetch_k <= 1024.
 * sim(i, j) is the f32 inner product of the STORED rows i and j: f16 / bf16 rows as stored, e4m3 rows decoded to
 * bf16 and scaled by 2^-s (what ts_index_reconstruct returns), f32 rows in exact f32 arithmetic; with the unit rows
 * the pipeline stores, the cosine.  Step 0 picks the largest relevance; step t picks the unpicked candidate with the
 * largest  lambda * rel_i - (1 - lambda) * max_{j picked} sim(i, j),  evaluated in f32 (each product rounded, then
 * the difference); ties go to the lower position in the candidate list.  Padding is never picked, nor is the id of
 * a removed (tombstoned) row: it is skipped like padding.  out_rel / out_ids [nq, k] hold the picks in selection
 * order, out_rel their relevances; the tail is -1 / -FLT_MAX where a query has fewer than k valid candidates.
 * lambda = 1 returns the first k valid candidates in relevance order (for a list ts_index_search returned: its
 * first k entries).
 * All pointers are device memory (host memory with TS_FLAG_HOST_PTR, staged; the call is then synchronous).  With
 * device pointers the call only enqueues three kernels per chunk of queries on `stream` (gather of the candidates'
 * 16-byte units into a tile, Gram matrix on the matrix cores, greedy selection) and returns: it chains behind a
 * ts_index_search on the same stream without a synchronisation.  Calls on one handle share its scratch (candidate
 * tiles and Gram matrices of one chunk of queries, at most 384 MiB whatever nq; allocated at the first call, freed
 * with the handle) and are ordered one behind the other.
 * TS_ERR_INVALID: null handle or pointer, k < 1, k > fetch_k, lambda outside [0, 1] (or NaN), and with
 * TS_FLAG_HOST_PTR an id other than -1 outside [offset, offset + ntotal).  Device ids cannot be read without a
 * synchronisation: there such an id is never dereferenced and is skipped like padding.  TS_ERR_UNSUPPORTED:
 * fetch_k > 1024.  Both before any HIP call, with a message in ts_last_error().
 * ts_mmr_ivf: the same over the rows of an IVF index (ids through its id-to-slot table on the device); bit for bit
 * what ts_index_mmr returns on a flat index of the same dtype holding the same rows.  (Outside the ts_ivf_ prefix
 * for the reason given at ts_remove_ivf.)                                                                        */
int ts_index_mmr(ts_index* h, const int64_t* cand_ids, const float* cand_rel, int32_t nq, int32_t fetch_k, int32_t k,
                 float lambda, float* out_rel, int64_t* out_ids, uint32_t flags, void* stream);
/* Measurement aid of tools/mmr_probe.py (no reference counterpart): with timing on, ts_index_mmr records HIP events
 * around the three kernels of every chunk and waits for each chunk, so the call is synchronous; ms[0..2] are the
 * summed milliseconds of gather, Gram and greedy selection over *calls timed calls since the last reset.           */
int ts_index_mmr_set_timing(ts_index* h, int32_t on);
int ts_index_mmr_get_timings(ts_index* h, double ms[3], int64_t* calls, int32_t reset);
/* ---- funnel search: rank on a prefix of the dimensions, rescore a shortlist exactly ----
 * Reference call site: none (the reference searches all dimensions; its stage-1 model is trained with Matryoshka
 * representation learning, so a prefix of its embedding is a usable embedding).  Added within version 4: no existing
 * signature or kernel changed, and a caller that never calls these allocates and launches nothing new.  f16 / bf16
 * storage only (TS_ERR_UNSUPPORTED otherwise).  Both calls are synchronous: they return with their stream drained.
 *
 * ts_index_search_prefix: ts_index_search_filtered on the inner product over the first `dims` components only.
 * `queries` holds nq rows of `dims` elements (q_dtype); stored rows are used as they are, nothing is renormalised.
 * The result is, bit for bit and id for id, what ts_index_search_filtered returns on an index of dimension `dims`
 * and the same storage dtype that holds the first `dims` components of every row under the same ids, with the same
 * rows removed: the same k groups of the same stored bytes in the same order; ties to the lower id; -1 / -FLT_MAX
 * padding; removed rows are never returned.  Masks as for ts_index_search_filtered, except that mask_of_query may be
 * NULL (no query has a mask).  The scan reads the first dims / 16 KiB of every 32-row block and nothing else of it.
 * dims % 128 == 0, 128 <= dims < dim, 1 <= k <= 16384; flags: TS_FLAG_HOST_PTR and TS_FLAG_NO_FILTER only; anything
 * else is TS_ERR_INVALID, before any HIP call.
 *
 * ts_index_rescore: exact full-dimension scores of given candidates.  queries [nq, dim] (q_dtype), cand_ids
 * [nq, ncand] int64 in the id space search returns, out_scores / out_ids [nq, k], all DEVICE memory;
 * 1 <= k <= ncand <= 16384.  Per query the valid candidates ordered by score descending, then id ascending; every
 * score is bit-identical to ts_index_scores / ts_index_search.  An entry that is -1, outside [offset, offset +
 * ntotal) or the id of a removed row has no rank: the tail of the output is -1 / -FLT_MAX.  An id given twice is
 * returned twice.  Calls on one handle share its scratch (candidate tiles of one chunk of queries, at most 384 MiB;
 * allocated at the first call, freed with the handle) and are serialised.
 * The funnel is ts_index_rescore of the ids ts_index_search_prefix returned, on one stream.
 * hip_stream: the hipStream_t the call runs on, what the other entry points call `stream`.  Both calls are held to
 * the synchronous stream contract, inputs arriving late on a side stream, by tests/test_stream_order_of_funnel_gpu.py; the table of
 * tests/stream_order.py lists the prototypes that spell the parameter `stream` and has no row for these two yet.  */
int ts_index_search_prefix(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t dims, int32_t k,
                           const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                           const int32_t* mask_of_query, float* out_scores, int64_t* out_ids, uint32_t flags,
                           void* hip_stream);
int ts_index_rescore(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, const int64_t* cand_ids,
                     int32_t ncand, int32_t k, float* out_scores, int64_t* out_ids, void* hip_stream);
/* ---- boosted search: a per-row score prior added inside the stage-1 scan ----
 * Reference call site: none (the reference ranks stage 1 by the inner product alone).  Added within version 4: no
 * existing signature or kernel changed, and a caller that never calls these allocates and launches nothing new.
 * f16 / bf16 storage only (TS_ERR_UNSUPPORTED otherwise).
 *
 * ts_index_search_biased: ts_index_search_filtered ranked on boosted(q, r) = fl32(score(q, r) + bias[r]).  score(q, r)
 * is exactly the float ts_index_search / ts_index_scores produce for the pair (the same query image, the same order of
 * the MFMA k groups); the addition is one IEEE f32 addition, round to nearest even, nothing fused or reassociated.
 * Per query the k allowed live rows with the largest boosted score, ties to the lower id, -1 / -FLT_MAX padding
 * where fewer than k rows are eligible; out_scores are the boosted scores, out_ids carry the id offset.  The result
 * is exact: a row with a modest score and a large bias is found, whatever its rank by score alone.  Masks as for
 * ts_index_search_filtered, except that mask_of_query may be NULL (no query has a mask); removed rows are never
 * returned.
 * bias: float32, entry r belongs to local row r (no id offset); bias_rows >= ntotal entries, of which exactly the first
 * ntotal are read, whatever ntotal % 32 is.  Device memory, 16-byte aligned, read in stream order on `hip_stream`; host
 * memory with TS_FLAG_HOST_PTR (any alignment).  One bias serves every query of the call.  Entries must be finite:
 * with TS_FLAG_HOST_PTR a NaN or an infinity is TS_ERR_INVALID; a device array is not checked: a row whose boosted
 * score is NaN is never returned, and the effect of an infinite entry is undefined (it may be returned or not, and
 * may cost the call its fast path).
 * Synchronous: the call returns with its stream drained; held coalesced passes are flushed first.  1 <= k <= 16384;
 * flags: TS_FLAG_HOST_PTR and TS_FLAG_NO_FILTER only.  A null pointer, bias_rows < ntotal, a bad mask argument, k out
 * of range or any other flag is TS_ERR_INVALID, before any HIP call.  Calls on one handle are serialised; the handle
 * keeps 128 bytes (plus a copy of the bias for host-pointer calls) from the first call on.
 * ts_index_last_bias_info, the last ts_index_search_biased on the handle: [0] passes (of at most 64 queries), [1]
 * passes whose first attempt was the fused path (thresholds, then the biased filter scan), [2] of those, passes redone
 * on the exact dense path (too few or too many candidates), [3] 32-row blocks its scans read.
 * hip_stream: the hipStream_t the call runs on, what the other entry points call `stream`.                        */
int ts_index_search_biased(ts_index* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k, const float* bias,
                           int64_t bias_rows, const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                           const int32_t* mask_of_query, float* out_scores, int64_t* out_ids, uint32_t flags,
                           void* hip_stream);
int ts_index_last_bias_info(const ts_index* h, int64_t info[4]);

/* ---- 4-bit MX index storage (TS_MXFP4_E2M1) -----------------------------------------------------
 * Half a byte per element plus one scale byte per 32 elements, scored in place.  A row is zero-padded to a multiple
 * of 64 dimensions; scale block (g, h), h = 0/1, holds the 32 dimensions k = 64 g + 16 m + 8 h + j (m = 0..3,
 * j = 0..7).  With amax the block's largest |x| (NaN counts as 0, +-Inf as +-FLT_MAX; with TS_FLAG_NORMALIZE x is the
 * f32 quotient x / (|x| + 1e-8)): e = 0 if amax == 0, else floor(log2 amax) - 2, plus 1 if amax > 6 * 2^e, clamped to
 * -100 .. 100; the scale byte is e + 127.  An element is its sign bit and the index of the value of
 * {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to |x| / 2^e (ties to the even index).  It decodes to sign * grid * 2^e, exact
 * in bf16.  Queries are rounded to bf16 whatever their dtype; a score equals, bit for bit, that of a TS_BF16 index
 * holding the decoded rows, and ts_index_reconstruct returns the decoded rows.  dim is at most 2048 (64-query passes up
 * to 1024).
 * Supported: add, reserve, reset, id offset, reconstruct, search (synchronous, asynchronous), search_filtered, scores,
 * grouped search, remove, compact, update.  TS_FLAG_ONE_LAUNCH, TS_FLAG_PIPELINE, TS_FLAG_COALESCE and the wide-pass
 * flags are ignored (ts_coalesce_groups* return 0 for it).  TS_ERR_UNSUPPORTED: range search, prefix search, rescore,
 * funnel search, boosted search, MMR; there is no IVF form.                                                        */
/* row-shard support: ids reported by search = local row + offset            */
int ts_index_set_id_offset(ts_index* h, int64_t offset);
/* copy rows [row0, row0+n) back out as row-major float32 (host or device):
 * used by save_index (reference src/stage1_retriever.py:421-441)            */
int ts_index_reconstruct(ts_index* h, int64_t row0, int64_t n, float* out,
                         uint32_t flags, void* stream);
/* counters of the last search on this handle: [0] path taken (low 4 bits: 0 dense,
 * 1 filter, 2 filter-then-dense fallback; +16 when the filter ran as the
 * one-launch scan), [1] max candidates per query, [2] sample rows,
 * [3] sample rank m.  After ts_index_range_search: see "range search".       */
int ts_index_last_search_info(const ts_index* h, int64_t info[4]);

/* Per-phase device timing of searches, measured with HIP events recorded on the
 * search's own stream (bench.py's roofline leg).  Phases: 0 query prep,
 * 1 sample scan, 2 thresholds, 3 fused scan+filter (the dominant kernel),
 * 4 candidate select, 5 dense path (scan+select), 6-7 unused.  ms[i] is the sum
 * over counts[i] occurrences since the last reset.  on = N > 1 times every N-th
 * search only (a timing event costs a few microseconds in the stream);
 * asynchronous searches record phase 3 only.                                 */
int ts_index_set_profiling(ts_index* h, int32_t on);
int ts_index_get_timings(ts_index* h, double ms[8], int64_t counts[8], int32_t reset);

/* Read-bandwidth ceiling of THIS box for the scan's access pattern (SURVEY.md 8d asks for a measured peak in
 * the same report as the roofline fraction): a kernel that only reads the index's tiled corpus — the scan's grid,
 * block order and non-temporal 16-byte loads, no LDS, no matrix cores, no epilogue — timed with HIP events on
 * `stream`, `reps` passes after one warm-up pass.  *bytes = bytes one pass reads (the algorithmic bytes of one
 * ts_index_search launch on this index).  No reference counterpart: measurement aid of bench.py.            */
int ts_index_read_probe(ts_index* h, int32_t reps, double* ms_avg, double* ms_best, int64_t* bytes,
                        void* stream);

/* ---- merge of per-shard partial top-k lists --------------------------------
 * New for the row-sharded multi-GPU path: `scores`/`ids` are
 * device arrays [nlists, nq, k] (e.g. the output of an RCCL all-gather of each
 * rank's ts_index_search result); writes the global top-k [nq, k] in the same
 * canonical order.  Entries with id < 0 are padding and ignored.  k <= 8192;
 * any number of lists (more than 16384 / k of them are merged in groups, then the
 * groups' results: the order is total, so the result is the same).
 * The order, as for ts_index_search: score descending with -0 equal to +0 (a
 * zero comes back as +0); NaN of either sign or payload below -inf (it comes
 * back as a NaN); exactly equal scores by ascending id, for any number of tied
 * entries and wherever they sit in the lists (the lists need not be sorted);
 * an id that occurs twice with one score occupies two places; the tail of a
 * query with fewer than k valid entries is id -1 / score -FLT_MAX, also where
 * the padding came in with another negative id.  The result does not depend
 * on the run.                                                                */
int ts_merge_topk(const float* scores, const int64_t* ids, int32_t nlists,
                  int32_t nq, int32_t k, float* out_scores, int64_t* out_ids,
                  int32_t device, void* stream);

/* Same, for lists that are not densely packed: list r's scores start at
 * scores + r*score_list_stride (floats) and its ids at ids + r*id_list_stride
 * (int64s) — e.g. each rank's [scores | ids] bytes gathered into one buffer, so
 * the merge reads the all-gather output in place.                            */
int ts_merge_topk_strided(const float* scores, const int64_t* ids, int32_t nlists,
                          int32_t nq, int32_t k, int64_t score_list_stride,
                          int64_t id_list_stride, float* out_scores, int64_t* out_ids,
                          int32_t device, void* stream);

/* ---- grouped search: top-k distinct groups of a ranked list ----
 * Reference call site: none (the reference returns the plain top-k of overlapping chunks, src/utils.py chunk_text);
 * what Milvus calls grouping search and Elasticsearch collapse.  Added within version 4: no existing signature or
 * kernel changed, and a caller that never calls it allocates and launches nothing new.  Stateless, like ts_merge_topk.
 * Per query: a candidate list of ncand entries, cand_ids [nq, ncand] int64 (-1 = padding) and cand_scores [nq, ncand]
 * float32, in rank order: the scores are carried, never compared.  groups [n_rows] int32 is shared by all queries;
 * entry `id` belongs to row id - id_base.
 *   valid      an entry with id != -1 and 0 <= id - id_base < n_rows.  Its group is groups[id - id_base]; a negative
 *              table value means "no group": the entry is a group of its own.
 *   selection  walking the list in position order, occ(i) = earlier valid entries of i's group, rank(i) = distinct
 *              groups whose first entry comes before the first entry of i's group; entry i is kept iff rank(i) < k and
 *              occ(i) < group_size.  An id that occurs twice counts twice.
 *   outputs    [nq, k * group_size]: out_scores, out_ids and out_groups (-1 for an entry without a group) of the kept
 *              entries in ascending list position (for a list ts_index_search returned: still in score order), then
 *              -FLT_MAX / -1 / -1.  out_ngroups [nq]: the distinct groups among ALL valid entries of the list (not
 *              capped at k); out_nvalid [nq]: its valid entries.
 * 1 <= ncand <= 16384, k >= 1, group_size >= 1, k * group_size <= 16384; k > ncand is allowed (the rest is padding).
 * The result depends neither on the run nor on nq.  With group_size > 1 over a list cut at ncand places, a group's
 * entries are its best WITHIN the list (the non-strict group size of Milvus): a later entry of the group that the
 * list does not hold cannot be returned.
 * All pointers, `groups` included, are device memory: the call enqueues one kernel (one workgroup per query, the
 * list sorted by (group, position) in LDS) on `stream` and returns, so it chains behind a ts_index_search on the
 * same stream without a synchronisation.  With TS_FLAG_HOST_PTR they are all host memory, staged through one device
 * allocation that is freed before the call returns, and the call is synchronous.
 * TS_ERR_INVALID: a null pointer, nq < 0, ncand < 1, k < 1, group_size < 1, n_rows < 0, and with TS_FLAG_HOST_PTR an
 * id other than -1 outside [id_base, id_base + n_rows) (nothing is written).  Device ids cannot be read without a
 * synchronisation: there such an id is range-checked on the device, never used as an index, and skipped like
 * padding (the convention of ts_index_mmr).  TS_ERR_UNSUPPORTED: ncand or k * group_size above 16384.  Both before
 * any HIP call, with a message in ts_last_error().  nq == 0 is TS_OK.                                            */
int ts_group_topk(const int64_t* cand_ids, const float* cand_scores, int32_t nq, int32_t ncand,
                  const int32_t* groups, int64_t n_rows, int64_t id_base, int32_t k, int32_t group_size,
                  float* out_scores, int64_t* out_ids, int32_t* out_groups,
                  int32_t* out_ngroups, int32_t* out_nvalid,
                  uint32_t flags, int32_t device, void* stream);

/* ---- stage-2 MaxSim ------------------------------------------------------
 * replaces ColBERTScorer._maxsim_score / _colbert_score applied per candidate
 * (reference src/stage2_rescorer.py:167-201, loop at :268-276).
 * q:       device [Lq, H] token embeddings of the query (dtype)
 * docs:    device [sum(Ld_i), H] token embeddings of all candidates, packed
 * doc_off: device int32 [n_docs+1] row offsets into docs
 * mode:    0 = maxsim (mean_i max_j cos), 1 = colbert (softmax-weighted)
 * out:     device float32 [n_docs]                                           */
int ts_maxsim(const void* q, int32_t Lq, const void* docs,
              const int32_t* doc_off, int32_t n_docs, int32_t H, int32_t dtype,
              int32_t mode, float* out, int32_t device, void* stream);

/* Same scores for candidates that already live in a resident token store
 * (token matrices computed once at add time instead of per query,
 * reference src/stage2_rescorer.py:254-259): document i occupies rows
 * [starts[i], starts[i]+lens[i]) of `store` [rows, H].  starts: device int64[n_docs],
 * lens: device int32[n_docs].  No gather copy: the kernel reads the store in place. */
int ts_maxsim_indexed(const void* q, int32_t Lq, const void* store, const int64_t* starts,
                      const int32_t* lens, int32_t n_docs, int32_t H, int32_t dtype,
                      int32_t mode, float* out, int32_t device, void* stream);

/* The same for several queries in ONE launch (the batched caller: RetrievalPipeline.search_many):
 * query j has tokens [q_off[j], q_off[j+1]) of q [sum Lq, H] and candidates
 * [cand_off[j], cand_off[j+1]) of starts / lens / out.  q_off and cand_off are HOST arrays of
 * nq+1 int32 starting at 0 (they travel inside the kernel arguments, 64 queries per launch, so the
 * caller may free them on return); everything else is device memory.  A single query's launch is
 * dominated by fixed costs (~25 of ~50 us at 1000 candidates); batched, they overlap with the
 * other queries' streaming.                                                              */
int ts_maxsim_indexed_batch(const void* q, const int32_t* q_off, int32_t nq, const void* store,
                            const int64_t* starts, const int32_t* lens, const int32_t* cand_off,
                            int32_t H, int32_t dtype, int32_t mode, float* out, int32_t device,
                            void* stream);

/* ---- stage-2 MaxSim over an e4m3 token store (added within ABI version 4: no existing signature changed) ----
 * The resident token store kept at one byte per element.  Stored format: a document token row x
 * (H elements) is the H bytes of OCP e4m3fn  e4m3_rne(x * 2^k),  k the largest integer with max|x_i| * 2^k <= 448
 * (max|x_i| * 2^k in (224, 448]); round to nearest even, e4m3 subnormals kept; a zero row stores zeros; a row with a
 * NaN or an Inf stores 0x7F in every byte.  k is not stored: the scores are cosines, which a positive per-row
 * factor does not change.
 *   ts_quantize_rows_fp8   x [rows, H] of x_dtype (TS_F32 / TS_F16 / TS_BF16) -> out [rows, H] bytes, in that
 *                          format bit for bit.  H % 16 == 0 and 16-byte aligned x / out, else TS_ERR_UNSUPPORTED.
 *   ts_maxsim_indexed_fp8, ts_maxsim_indexed_batch_fp8
 *                          ts_maxsim_indexed / _batch over such a store: the query stays q_dtype (TS_F16 /
 *                          TS_BF16), the store's bytes are converted in registers (exactly: every e4m3 value is a
 *                          bf16 and an f16 value), so the scores are the exact cosines of the decoded rows against
 *                          the query.  H % 16 != 0, or a query image over the kernel's LDS budget (H > 2048 at
 *                          the time of writing): TS_ERR_UNSUPPORTED — there is no general kernel behind these.
 *                          Lq >= 1 (q_off strictly increasing where a query has candidates).  Existing entry
 *                          points keep rejecting dtype TS_FP8_E4M3.                                           */
int ts_quantize_rows_fp8(const void* x, int32_t x_dtype, int64_t rows, int32_t H, void* out, int32_t device,
                         void* stream);
int ts_maxsim_indexed_fp8(const void* q, int32_t q_dtype, int32_t Lq, const void* store, const int64_t* starts,
                          const int32_t* lens, int32_t n_docs, int32_t H, int32_t mode, float* out, int32_t device,
                          void* stream);
int ts_maxsim_indexed_batch_fp8(const void* q, int32_t q_dtype, const int32_t* q_off, int32_t nq, const void* store,
                                const int64_t* starts, const int32_t* lens, const int32_t* cand_off, int32_t H,
                                int32_t mode, float* out, int32_t device, void* stream);

/* ---- best passage per candidate: windowed MaxSim over the token store (added within ABI version 4) ----
 * Extends the reference's MaxSim (src/stage2_rescorer.py:167-183), which scores a whole chunk, by saying which part
 * of the chunk matched.  Query token rows q_t, t < Lq, 1 <= Lq <= 256; candidate i's token rows x_j, j < Ld, are
 * rows [starts[i], starts[i] + lens[i]) of `store`; c[t][j] is the cosine of q_t and x_j formed as ts_maxsim_indexed
 * forms it (f32 accumulation of the stored values, the same normalisation, a zero row gives 0).  For a window of
 * `window` >= 1 tokens:
 *   we = min(window, Ld);  positions p in [0, Ld - we];  S[p] = sum over t of max_{p <= j < p + we} c[t][j]  (f32,
 *   added in ascending t: deterministic, no float atomics, two runs give the same bits);
 *   p* = the position with the largest S[p], compared as f32, ties to the lowest p, a NaN sum last.
 *   out_start[i] = p*,  out_len[i] = we,  out_score[i] = S[p*] / Lq  (one f32 division: the mean of `maxsim` mode;
 *   there is no `colbert` form of this call);
 *   out_align (may be NULL) [i][t] = the j in [p*, p* + we) with the largest c[t][j], ties to the lowest j, as a
 *   position in the document.
 * With window >= Ld the window is the document and out_score is ts_maxsim_indexed's `maxsim` score of the candidate:
 * bit for bit where the sums are exact, within rounding of a sum of Lq cosines otherwise.
 * A candidate with lens[i] <= 0 gets start -1, length 0, score -FLT_MAX and alignment -1 (ts_maxsim_indexed gives
 * such a candidate the score 0.0, the reference's value for a candidate that cannot be scored).  lens is device memory
 * and these calls do not synchronise, so a candidate of more than 1024 rows is refused where it is met: the call
 * returns TS_OK and that candidate gets start -2 (not -1), length 0, score -FLT_MAX and alignment -1 (the Python
 * wrappers check the lengths and raise before the launch).  Candidates of 193 .. 1024 rows are taken by a second
 * kernel of at most 1024 workgroups, one workgroup per CU at a time: they cost more per row than shorter ones.
 * The batch form follows ts_maxsim_indexed_batch: q_off and cand_off are HOST arrays of nq + 1 int32 starting at 0;
 * row cand_off[j] + i of out_align has align_ld >= max Lq entries, those at t >= Lq_j are -1; the single form's rows
 * have Lq entries.  Both run on the caller's stream without host synchronisation.
 * TS_ERR_INVALID (before any HIP call): a null pointer other than out_align, window < 1, H < 1, Lq < 1 (a query
 * with candidates and no tokens), a negative count, decreasing offsets, align_ld below the longest query.
 * TS_ERR_UNSUPPORTED (before any HIP call): Lq > 256, rows whose size H * element size is no multiple of 16 bytes,
 * q or store not 16-byte aligned, dtype TS_FP8_E4M3 (an e4m3 token store is out of scope).  Store types: TS_F16,
 * TS_BF16, TS_F32; q has the store's type.  n_docs == 0 / nq == 0 is TS_OK.                                     */
int ts_maxsim_passages_indexed(const void* q, int32_t Lq, const void* store, const int64_t* starts,
                               const int32_t* lens, int32_t n_docs, int32_t H, int32_t dtype, int32_t window,
                               int32_t* out_start, int32_t* out_len, float* out_score, int32_t* out_align,
                               int32_t device, void* stream);
int ts_maxsim_passages_indexed_batch(const void* q, const int32_t* q_off, int32_t nq, const void* store,
                                     const int64_t* starts, const int32_t* lens, const int32_t* cand_off, int32_t H,
                                     int32_t dtype, int32_t window, int32_t* out_start, int32_t* out_len,
                                     float* out_score, int32_t* out_align, int32_t align_ld, int32_t device,
                                     void* stream);

/* ---- BM25 (the lexical half of stage 1) ---------------------------------------
 * replaces BM25Index.search (reference src/stage1_retriever.py:103-112, called at
 * :385-388): same float64 arithmetic and ordering (score desc, doc id asc), but the
 * postings live in HBM (CSR) and a query touches only its terms' postings.
 * ts_bm25_set_index takes HOST arrays: term_off[V+1], post_doc/post_tf[nnz] sorted
 * by term, idf[V], len_norm[N] = k1*(1-b+b*len/avg), k1p1 = k1+1.
 * ts_bm25_search: term_ids = query tokens as vocabulary ids in query order (host);
 * writes (score, doc) pairs to HOST arrays: the first min(k, T) of the T documents the
 * query TOUCHES (those in the postings of at least one of its terms), by score desc, doc
 * id asc, and *n_out = min(k, T); k <= 2048, TS_ERR_UNSUPPORTED above.  Untouched
 * documents score exactly 0.0 and are never written.  With every idf > 0 a touched
 * document scores above 0.0, so *n_out < k means all documents with a non-zero score were
 * returned.  With an idf <= 0 a touched document may score 0.0 (written as +0.0) or less:
 * it is still written, once, and ranking it against the untouched documents (which then
 * tie with it or beat it) is left to the caller.  A ts_bm25
 * handle keeps ONE set of accumulator / candidate workspaces: calls on one handle must
 * not overlap (one caller at a time; different handles are independent).        */
typedef struct ts_bm25 ts_bm25;
int ts_bm25_create(int32_t device, ts_bm25** out);
int ts_bm25_destroy(ts_bm25* h);
int ts_bm25_set_index(ts_bm25* h, int64_t N, int64_t V, int64_t nnz, const int64_t* term_off,
                      const int32_t* post_doc, const float* post_tf, const double* idf,
                      const double* len_norm, double k1p1);
int ts_bm25_search(ts_bm25* h, const int32_t* term_ids, int32_t n_terms, int32_t k,
                   double* out_scores, int64_t* out_ids, int32_t* n_out, void* stream);
/* The same for nq queries with ONE synchronisation: query q's terms are
 * term_ids[term_off[q] .. term_off[q+1]) (host arrays; term_off has nq+1 entries), its
 * results out_scores / out_ids [q*k .. q*k + n_out[q]).  Each query is scored exactly as by
 * ts_bm25_search (same kernels, same order of additions per query); the queries of a batch
 * run side by side — one launch per token position for up to 64 of them, each with its own
 * accumulator (20 bytes per document and query, at most 4 GiB per handle) — instead of one
 * chain of launches per query.                                                           */
int ts_bm25_search_batch(ts_bm25* h, const int32_t* term_ids, const int64_t* term_off, int32_t nq,
                         int32_t k, double* out_scores, int64_t* out_ids, int32_t* n_out,
                         void* stream);
/* ts_bm25_search_batch restricted per query to an allowed set of documents (the masks of
 * ts_index_search_filtered: n_masks masks of allow_words >= ceil(N / 32) words, bit d % 32 of word d / 32 =
 * document d allowed; mask_of_query a HOST array, -1 = not filtered).  allow_bits is device memory, host memory
 * with TS_FLAG_HOST_PTR.  A document outside its query's mask is never scored or touched: the output holds the
 * allowed touched documents only (*n_out < k: all of them), so a caller's zero-score padding must take
 * allowed documents too.  Allowed documents score exactly as in ts_bm25_search_batch.                      */
int ts_bm25_search_batch_filtered(ts_bm25* h, const int32_t* term_ids, const int64_t* term_off, int32_t nq,
                                  int32_t k, const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks,
                                  const int32_t* mask_of_query, uint32_t flags, double* out_scores,
                                  int64_t* out_ids, int32_t* n_out, void* stream);

/* ---- fused residual add + LayerNorm (between the GEMMs of the encoder forwards) ---
 * The cross-encoder forward the reference reaches through CrossEncoder.predict
 * (src/stage3_reranker.py:127-131) is PyTorch-ROCm GEMMs and attention here too; the
 * residual add, LayerNorm and the cast for the next GEMM between them are one pass:
 *   y = LayerNorm(x + residual) * gamma + beta  over the last dimension H (fp32
 *   statistics and arithmetic, like torch.layer_norm);
 * x [rows, H] of x_dtype; residual fp32 [rows, H] or NULL; gamma / beta fp32 [H];
 * y is written as fp32 (out_f32, may be NULL) and / or in lp_dtype (out_lp, TS_F16 or
 * TS_BF16, may be NULL).  beta may be NULL (a LayerNorm without bias).  H a multiple of
 * 4, <= 2048; pointers 16-byte aligned (device).                                    */
int ts_add_layernorm(const void* x, int32_t x_dtype, const float* residual, const float* gamma,
                     const float* beta, float eps, int64_t rows, int32_t H, float* out_f32,
                     void* out_lp, int32_t lp_dtype, int32_t device, void* stream);

/* The same pass for a pre-LN model (ModernBERT, the reference's default stage-2 token
 * encoder, src/stage2_rescorer.py:30): out_sum (fp32, may be NULL) receives x + residual
 * — the residual stream — and out_lp the normalised row for the next GEMM.           */
int ts_add_prenorm(const void* x, int32_t x_dtype, const float* residual, const float* gamma,
                   const float* beta, float eps, int64_t rows, int32_t H, float* out_sum,
                   void* out_lp, int32_t lp_dtype, int32_t device, void* stream);

/* The embedding layer of those models the same way: row r of the output is
 *   LayerNorm((word[ids[r]] + type[type_ids[r]]) + position[pos_ids[r]]) * gamma + beta
 * (the order of additions of BertEmbeddings / RobertaEmbeddings); ids / pos_ids /
 * type_ids int64 [rows] on the device (type_ids NULL = type 0), tables fp32 [*, H]
 * — indices are NOT range checked; outputs as for ts_add_layernorm.                */
int ts_embed_layernorm(const int64_t* ids, const int64_t* pos_ids, const int64_t* type_ids,
                       const float* word_tab, const float* pos_tab, const float* typ_tab,
                       const float* gamma, const float* beta, float eps, int64_t rows, int32_t H,
                       float* out_f32, void* out_lp, int32_t lp_dtype, int32_t device, void* stream);

/* ---- self-attention of a right-padded batch (the attention of those forwards) -----
 * softmax(Q K^T * scale) V per head over the first lens[b] tokens of sequence b only —
 * what torch's scaled_dot_product_attention computes under the padding mask of
 * CrossEncoder.predict's tokenizer batch (src/stage3_reranker.py:127-131), without
 * a mask tensor and without work on the padding.  qkv [B, L, 3, heads, dh] of dtype
 * (TS_F16 / TS_BF16): the output of the fused Q/K/V projection, read in place;
 * lens int32 [B] (device; clamped to L; 0 = nothing written for that sequence);
 * out [B, L, heads*dh] of dtype — rows at padded positions are NOT written.  fp32
 * softmax statistics and accumulation, probabilities rounded to dtype before the
 * P V product (as flash attention does).  dh 32 or 64; K and V^T of one sequence and
 * head must fit the 160 KB of LDS: L <= 1120 at dh 32, L <= 576 at dh 64;
 * pointers 16-byte aligned, B <= 65535.  window > 0: query q only sees the keys k with
 * |q - k| <= window (the bidirectional sliding window of ModernBERT's local layers:
 * window = local_attention / 2); 0 = all keys.  rope_cos / rope_sin (fp32 [L, dh], both or
 * neither): the rotary embedding of ts_rope_inplace applied to q and k as they are
 * loaded — same arithmetic, same results as ts_rope_inplace followed by this call
 * without tables, minus one pass over q and k (qkv itself is left as it is).
 * offs (int32 [B] on the device, or NULL): a PACKED batch — qkv is [T, 3, heads, dh] and out
 * [T, heads*dh] with sequence b occupying tokens offs[b] .. offs[b] + lens[b]; L is then
 * only the upper bound of lens (it sizes the LDS tiles).  NULL: the padded layout above.  */
int ts_attention_varlen(const void* qkv, const int32_t* lens, int32_t B, int32_t L, int32_t heads,
                        int32_t dh, int32_t dtype, float scale, int32_t window,
                        const float* rope_cos, const float* rope_sin, const int32_t* offs, void* out,
                        int32_t device, void* stream);

/* Rotary position embedding of the q and k thirds of qkv [B, L, 3, heads, dh] in place:
 * x <- x * cos + rotate_half(x) * sin with fp32 tables cos / sin [L, dh] (row = token
 * position), computed in fp32 like transformers' apply_rotary_pos_emb (products and sum
 * each rounded, no fused multiply-add), rounded once to dtype.  dh a multiple of 8.   */
int ts_rope_inplace(void* qkv, int32_t dtype, const float* cos_tab, const float* sin_tab, int64_t B,
                    int32_t L, int32_t heads, int32_t dh, int32_t device, void* stream);

/* Gated GELU of ModernBertMLP: u [rows, 2 I] -> out [rows, I] = gelu(u[:, :I]) * u[:, I:]
 * (erf GELU in fp32 rounded to dtype, then the product rounded to dtype: the two
 * roundings of the two torch ops).  I a multiple of 8.                               */
int ts_geglu(const void* u, int32_t dtype, int64_t rows, int32_t I, void* out, int32_t device,
             void* stream);

/* ---- linear layers with a short reduction dimension (the projections of those forwards) ---
 * out[M, N] = act(x[M, K] w[N, K]^T + bias[N]) for the Q/K/V, attention-output and feed-
 * forward "up" projections of MiniLM-class encoders (K <= 384 is where it beats the
 * library GEMM, 1.2-1.5x; at K = 768 hipBLASLt's stream-K kernels win and the Python
 * host keeps them; any K that is a multiple of 128 up to 2176 is accepted), act 0 = none,
 * 1 = erf GELU (BertIntermediate: no separate activation pass over the M x N result).
 * The weight is re-tiled ONCE with ts_linear_tile_weight (w [N, K] in torch.nn.Linear
 * layout -> out, N*K elements of the same dtype) and then streamed from L2 by every
 * workgroup while the workgroup's rows of x sit in LDS (the structure of the stage-1 scan,
 * DESIGN.md 4.7).  x, bias (may be NULL), out of dtype (TS_F16 / TS_BF16), fp32 accumulation;
 * sum + bias is rounded to dtype before the activation, the result rounded again — the
 * roundings of linear followed by gelu.  N a multiple of 32; pointers 16-byte aligned
 * (bias 8).                                                                              */
int ts_linear_tile_weight(const void* w, int32_t dtype, int32_t N, int32_t K, void* out,
                          int32_t device, void* stream);
int ts_linear_act(const void* w_tiled, const void* x, const void* bias, int32_t dtype, int64_t M,
                  int32_t N, int32_t K, int32_t act, void* out, int32_t device, void* stream);

/* BertSelfOutput / BertOutput of a post-LN encoder in ONE kernel (the cross-encoder the reference reaches through
 * CrossEncoder.predict, /root/reference/src/stage3_reranker.py:127-131; transformers' modeling_bert
 * BertSelfOutput.forward / BertOutput.forward: dense -> dropout -> LayerNorm(hidden + input)):
 *     y = LayerNorm(round_dtype(a(x)[M, K] w[N, K]^T + bias[N]) + residual[M, N]) * gamma + beta
 * w_tiled from ts_linear_tile_weight; x, bias (may be NULL) of dtype (TS_F16 / TS_BF16); residual fp32 (may be
 * NULL), gamma fp32 [N], beta fp32 [N] or NULL; y is written as fp32 (out_f32, the next residual) and / or in
 * dtype (out_lp, the next GEMM's input) — at least one of them.  act_in 0: a(x) = x; 1: a(x) = round_dtype(
 * erf GELU(x)) applied as the rows are staged — BertIntermediate's activation folded into BertOutput, x being
 * the up projection's output BEFORE its activation (ts_linear_act with act 0): the activation costs no pass
 * of its own and its arithmetic runs beside this kernel's matrix instructions.  The roundings are those of
 * (gelu,) ts_linear_act, ts_add_layernorm, and for N > 128 so are the bits (below, the fp32 row statistics may
 * differ in the last place: 1e-6).  N a multiple of 32 up to 384 (a workgroup owns
 * whole rows: the projection's output never goes to HBM), K a multiple of 384; pointers 16-byte aligned (bias 8). */
int ts_linear_add_layernorm(const void* w_tiled, const void* x, const void* bias, const float* residual,
                            const float* gamma, const float* beta, float eps, int32_t dtype, int64_t M,
                            int32_t N, int32_t K, int32_t act_in, float* out_f32, void* out_lp, int32_t device,
                            void* stream);

/* BertIntermediate + BertOutput — the whole feed-forward block of a post-LN encoder layer — in ONE kernel:
 *     y = LayerNorm(round(gelu(round(x[M, H] w1[I, H]^T + b1[I])) w2[H, I]^T + b2[H]) + residual[M, H]) * gamma + beta
 * (erf GELU; round = to dtype).  The M x I intermediate never leaves the CU (as separate kernels it is written to HBM
 * and read back: 40 % of a layer's traffic).  w1_tiled / w2_tiled from ts_linear_tile_weight; x, b1, b2 (may be
 * NULL) of dtype (TS_F16 / TS_BF16); residual fp32 (may be NULL), gamma fp32 [H], beta fp32 [H] or NULL; outputs as
 * for ts_linear_add_layernorm.  The roundings and the accumulation order are those of ts_linear_act (act 1) followed
 * by ts_linear_add_layernorm: the same bits.  H = 384 (MiniLM-class: a workgroup owns whole rows), I a multiple of
 * 384; pointers 16-byte aligned (biases 8).                                                                     */
int ts_mlp_add_layernorm(const void* w1_tiled, const void* b1, const void* w2_tiled, const void* b2, const void* x,
                         const float* residual, const float* gamma, const float* beta, float eps, int32_t dtype,
                         int64_t M, int32_t H, int32_t I, float* out_f32, void* out_lp, int32_t device, void* stream);

/* Frees the internal MaxSim scratch buffers kept per (device, stream) (all devices
 * if device < 0).  No MaxSim launch may be pending on that device.               */
int ts_maxsim_release_scratch(int32_t device);

/* ---- IVF-Flat -----------------------------------------------------------------
 * replaces faiss.IndexIVFFlat(quantizer, d, nlist, METRIC_INNER_PRODUCT) with nprobe (reference
 * src/stage1_retriever.py:256-283).  Inner product only; f16 / bf16 storage in 32-row blocks that each hold rows of
 * one inverted list; an fp32 flat index of the centroids is the coarse quantizer.  Every pointer except
 * ts_ivf_list_sizes's and ts_ivf_train's `objective` (host) is device memory on the handle's device.  A handle serves
 * one caller at a time.  Added within ABI version 4: no existing signature changed.
 *   train     spherical k-means on <= 256 * nlist points sampled with `seed` (initial centroids: the first nlist of
 *             them), `iters` iterations, centroids L2-normalised after each update, an empty cluster re-seeded by
 *             splitting the largest; deterministic (no float atomics).  n < nlist: TS_ERR_INVALID.  objective
 *             (NULL or host double[iters]) receives the sum of each point's best centroid score per iteration.
 *   add       each row (after the flat index's rounding and optional normalisation) goes to the list of its highest
 *             fp32 centroid score, ties to the lower list; ids are insertion order plus the id offset.  Before
 *             train / set_centroids: TS_ERR_INVALID.
 *   probe     the nprobe lists of highest fp32 centroid score, descending, ties to the lower list id.
 *   search    the exact top-k over the rows of the query's probed lists (scores bit-identical to ts_index_search on
 *             the same rows, ties by ascending id), -1 / -FLT_MAX padded; synchronous with respect to `stream`.
 *   reconstruct  rows [id0, id0 + n) in id order as float32.
 *   last_search_info  {passes, passes on the filter path, of them redone densely, live blocks of the last pass}. */
typedef struct ts_ivf ts_ivf; /* opaque */
int ts_ivf_create(int32_t dim, int32_t nlist, int32_t storage_dtype, int32_t device, ts_ivf** out);
int ts_ivf_destroy(ts_ivf* h);
int ts_ivf_reset(ts_ivf* h);   /* drop all rows, keep the centroids */
int ts_ivf_train(ts_ivf* h, const void* x, int64_t n, int32_t x_dtype, int64_t seed, int32_t iters,
                 double* objective, void* stream);
int ts_ivf_set_centroids(ts_ivf* h, const float* centroids, void* stream);   /* [nlist, dim] fp32, empty index */
int ts_ivf_get_centroids(ts_ivf* h, float* out, void* stream);
int32_t ts_ivf_is_trained(const ts_ivf* h);
int ts_ivf_add(ts_ivf* h, const void* rows, int64_t n, int32_t rows_dtype, uint32_t flags, void* stream);
int ts_ivf_search(ts_ivf* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t k, int32_t nprobe,
                  float* out_scores, int64_t* out_ids, void* stream);
int ts_ivf_probe(ts_ivf* h, const void* queries, int32_t nq, int32_t q_dtype, int32_t nprobe, float* out_scores,
                 int64_t* out_lists, void* stream);
int ts_ivf_list_sizes(const ts_ivf* h, int64_t* out);   /* host int64[nlist] */
int ts_ivf_reconstruct(ts_ivf* h, int64_t id0, int64_t n, float* out, void* stream);
int64_t ts_ivf_ntotal(const ts_ivf* h);
/* removal, with the contract of ts_index_remove (ids as search returns them, HOST int64[n]; unknown, repeated and
 * removed ids not counted): the slot leaves its block's valid bits, so the scan and the thresholds (whose N_q counts
 * live probed rows) never see it again, and its list shrinks (ts_ivf_list_sizes counts live rows).  The hole stays
 * until ts_compact_ivf; reconstruct still returns the stored row.  Added within version 4.                        */
/* (outside the ts_ivf_ prefix: that set of entry points is fixed by the IVF ABI tests) */
int ts_remove_ivf(ts_ivf* h, const int64_t* ids, int64_t n, int64_t* n_removed, void* stream);
/* update in place, with the contract of ts_index_update (all or nothing; rows DEVICE only, as ts_ivf_add).  Reference
 * call site: none (the reference never changes a stored vector).  Each row leaves its list exactly as ts_remove_ivf
 * makes it leave, is assigned by the quantizer exactly as ts_ivf_add assigns a new row, and is placed at the end of
 * its new list under its old id; ntotal does not change and the hole stays, as after a removal, until
 * ts_compact_ivf.  Added within version 4; outside the ts_ivf_ prefix for the reason given above.                 */
int ts_update_ivf(ts_ivf* h, const int64_t* ids, int64_t n, const void* rows, int32_t rows_dtype, uint32_t flags,
                  void* stream);
/* compaction, with the contract of ts_index_compact: the live rows are renumbered densely in ascending id order,
 * ntotal = live rows afterwards, and old2new (HOST int64[old ntotal] of ids before the id offset, -1 = removed; may be
 * NULL) receives the monotone map.  The id offset and the centroids stay, and the quantizer is not run: a row stays in
 * the list it is in.  The survivors are placed as ts_ivf_add places rows (in id order, each the next slot of its list,
 * a list whose last block is full takes the next fresh block), so the index afterwards is the one a fresh handle with
 * the same centroids holds after one add of the surviving rows: the same list sizes, blocks, reconstructed rows and
 * search results bit for bit, now and after any later add / remove / update.  The holes of ts_update_ivf are closed
 * too (the map is then the identity); an index without a hole is left untouched, one with no live row is left empty
 * and trained.  All or nothing: the new corpus and tables are built beside the old ones (peak device memory: old +
 * new corpus) and swapped in at the end; on an error the index is as it was.  Ordered on `stream`, synchronous.
 * Added within version 4; outside the ts_ivf_ prefix for the reason given above.                                  */
int ts_compact_ivf(ts_ivf* h, int64_t* old2new, void* stream);
/* ts_index_mmr over an IVF index: see "diversified selection" above */
int ts_mmr_ivf(ts_ivf* h, const int64_t* cand_ids, const float* cand_rel, int32_t nq, int32_t fetch_k, int32_t k,
               float lambda, float* out_rel, int64_t* out_ids, uint32_t flags, void* stream);
int ts_ivf_set_id_offset(ts_ivf* h, int64_t offset);
int ts_ivf_last_search_info(const ts_ivf* h, int64_t info[4]);

/* ---- diagnostics (no GPU needed) -------------------------------------------
 * Exercises the per-device one-time table that guards hipFuncSetAttribute with
 * n_threads racing host threads over n_devices device numbers; 0 = every
 * (kernel, device) action ran exactly once, failed actions were retried.      */
int ts_selftest_device_once(int32_t n_threads, int32_t n_devices);

/* ---- misc ---------------------------------------------------------------- */
const char* ts_last_error(void);
int ts_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TRISTAGE_H_ */
