/* quickwit_amd — C-ABI for the MI355X-native Quickwit leaf-search hot path.
 *
 * This is the drop-in boundary of SURVEY.md §8b: it replaces the work the
 * reference ships to its rayon pool inside `leaf_search_single_split`
 * (quickwit/quickwit-search/src/leaf.rs:899-959), speaking the protobuf
 * messages of quickwit-proto/protos/quickwit/search.proto verbatim:
 *   - qw_leaf_search:  LeafSearchRequest (search.proto:362) in,
 *                      LeafSearchResponse (search.proto:618) out.
 *   - qw_ctx mirrors SearcherContext (quickwit-search/src/service.rs:405-427)
 *     for the fields that affect results/limits.
 * A Rust host binds these with a plain extern "C" block (INTEGRATION.md shows
 * the binding that would sit under leaf.rs:900).
 *
 * Ownership: request/split buffers are caller-owned and immutable for the
 * call; response buffers are callee-allocated and freed with qw_buf_free.
 * Errors: negative status + UTF-8 message via qw_last_error, mapped onto the
 * reference's SearchError variants; per-split failures are reported INSIDE
 * the response (LeafSearchResponse.failed_splits, search.proto:626), exactly
 * as the reference does (leaf.rs:2143-2147).
 */
#ifndef QUICKWIT_AMD_H
#define QUICKWIT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qw_ctx qw_ctx;

typedef struct qw_buf {
    uint8_t* data;
    size_t len;
} qw_buf;

/* Status codes (negative = error), mapped onto quickwit SearchError
 * (quickwit-search/src/error.rs). */
enum qw_status {
    QW_OK = 0,
    QW_ERR_INVALID_ARGUMENT = -1, /* SearchError::InvalidArgument */
    QW_ERR_INVALID_QUERY = -2,    /* SearchError::InvalidQuery */
    QW_ERR_NOT_FOUND = -3,        /* unknown split id */
    QW_ERR_INTERNAL = -4,         /* SearchError::Internal */
    QW_ERR_NO_GPU = -5,           /* no HIP device: the product path never
                                     falls back to CPU */
    QW_ERR_BAD_SPLIT = -6,        /* malformed QWA1 container */
    QW_ERR_OVER_MEMORY_BUDGET = -7, /* HBM budget refusal: the permit-provider
                                     * memory gate (search_permit_provider.rs:
                                     * 43-110) mapped to a synchronous C-ABI —
                                     * refuse instead of queueing */
};

/* config_json mirrors the result-affecting subset of SearcherConfig
 * (quickwit-config/src/node_config/mod.rs:408-461) plus device placement:
 *   {"device": 0,                       // HIP device ordinal
 *    "aggregation_memory_limit": 500000000,
 *    "aggregation_bucket_limit": 65000}
 * NULL/empty means defaults (device 0). Creation succeeds without a GPU;
 * device init is lazy (first add_split/search touching the device fails with
 * QW_ERR_NO_GPU instead). */
qw_ctx* qw_ctx_create(const char* config_json);
void qw_ctx_free(qw_ctx* ctx);

/* Register a split (QWA1 container bytes) and upload its sections to device
 * HBM — the analog of the reference's warmup having populated the
 * ByteRangeCache (leaf.rs:302-377): after this call the split is "warm" and
 * qw_leaf_search times pure search, like cpu_search_microsecs
 * (leaf.rs:905-946). The data buffer may be released by the caller after
 * return. */
int32_t qw_ctx_add_split(qw_ctx* ctx, const char* split_id,
                         const uint8_t* data, size_t len);
int32_t qw_ctx_remove_split(qw_ctx* ctx, const char* split_id);

/* LeafSearchRequest protobuf in, LeafSearchResponse protobuf out.
 * Splits referenced by LeafRequestRef.split_offsets must have been added.
 * Synchronous; internally one HIP stream per split. */
int32_t qw_leaf_search(qw_ctx* ctx, const uint8_t* leaf_search_request_pb,
                       size_t len, qw_buf* response_pb_out);

void qw_buf_free(qw_buf* buf);

/* fetch_docs phase 2 (quickwit-search/src/fetch_docs.rs; root.rs:903):
 * FetchDocsRequest protobuf in (search.proto:674), FetchDocsResponse out
 * (:695). Fetches the stored documents for the given PartialHits from the
 * splits' row store (zlib blocks + doc->block index);
 * leaf_json is the ingested document's canonical JSON. Snippets
 * (snippet_request) are not produced in round 1. Hits are returned grouped
 * by (split_id, doc_id) — the root matches them by partial_hit. */
int32_t qw_fetch_docs(qw_ctx* ctx, const uint8_t* fetch_docs_request_pb,
                      size_t len, qw_buf* response_pb_out);

/* leaf_list_terms (quickwit-search/src/list_terms.rs:211-322):
 * LeafListTermsRequest protobuf in (search.proto:732), LeafListTermsResponse
 * out (search.proto:745). Per split: sorted term-dictionary range scan over
 * [start_key, end_key) limited to max_hits, then k-merge + dedup across
 * splits. Term bytes are the RAW term value bytes (declared deviation: the
 * reference prefixes tantivy's serialized-Term header, an engine-internal
 * encoding with no analog here — DESIGN.md §7). Host-only (term dictionaries
 * stay on CPU); splits must have been added. */
int32_t qw_leaf_list_terms(qw_ctx* ctx, const uint8_t* leaf_list_terms_request_pb,
                           size_t len, qw_buf* response_pb_out);

/* Root-side helpers replacing the reference's tantivy-side merge
 * (collector.rs:832-861 merge_fruits / aggregation merge): merge N
 * LeafSearchResponse protobufs (top-K with reference tie-breaks + QAGG1
 * aggregation blobs + counters) into one, honoring the SearchRequest's
 * sort/max_hits. */
int32_t qw_merge_leaf_responses(const uint8_t* search_request_pb,
                                size_t search_request_len,
                                const uint8_t** response_pbs,
                                const size_t* response_lens, size_t n,
                                qw_buf* merged_out);

/* Merge N intermediate aggregation blobs (QAGG1) of one aggregation request
 * by key, as qw_merge_leaf_responses does for the blobs its responses carry;
 * n == 1 decodes and re-encodes. Ctx-less, host-only. */
int32_t qw_merge_intermediate_aggs(const uint8_t** blobs, const size_t* lens,
                                   size_t n, qw_buf* merged_out);

/* Finalize an intermediate aggregation blob (QAGG1) into the ES-shaped JSON
 * the reference's root returns for the same aggregation request. */
int32_t qw_finalize_agg_to_json(const uint8_t* blob, size_t len,
                                const char* agg_request_json,
                                qw_buf* json_out);

/* Regex over a packed term list, on the host, without a ctx or a GPU: the
 * same byte DFA (csrc/qregex.h) a regex query scans a split's dictionary
 * with on the device. Term t is term_bytes[term_offsets[t] ..
 * term_offsets[t+1]); term_offsets has num_terms + 1 entries. Sets bit t % 64
 * of match_bitmap_out[t / 64] iff the WHOLE term matches; the caller provides
 * (num_terms + 63) / 64 words, all of which are written. The regex is taken
 * as given (no automatic "(?i)"). A refused or malformed regex returns
 * QW_ERR_INVALID_QUERY with the construct named in qw_last_error(NULL). */
int32_t qw_regex_match_terms(const char* regex, size_t regex_len,
                             const uint8_t* term_bytes,
                             const uint32_t* term_offsets, size_t num_terms,
                             uint64_t* match_bitmap_out);

/* Size of the DFA a regex compiles to: out[0] = states (dead state
 * included), out[1] = byte classes, out[2] = bytes of the table image the
 * device reads (k_dict_dfa_match stages it in LDS up to 64 KB and reads it
 * from global memory above). Errors as qw_regex_match_terms. */
int32_t qw_regex_table_stats(const char* regex, size_t regex_len,
                             uint64_t out[3]);

/* The regex a regex query on a field evaluates: "(?i)" is prepended when the
 * field's tokenizer lowercases, unless a leading flag group already carries
 * `i` (RegexQuery::to_resolved, query_ast/regex_query.rs). */
int32_t qw_regex_resolve(const char* regex, size_t regex_len,
                         int32_t tokenizer_lowercases, qw_buf* resolved_out);

/* Last error message for this ctx (UTF-8, valid until next call on ctx).
 * For ctx-less entry points (merge/finalize), pass NULL to read the
 * thread-local message. */
const char* qw_last_error(const qw_ctx* ctx);

/* ---- instrumentation (bench/roofline; not part of the reference surface) */

/* Accumulated device time (HIP events on the launch stream) and launch count
 * for a named kernel since the last reset. Returns QW_ERR_NOT_FOUND for an
 * unknown name. Known names: "union_bm25", "range_filter", "column_agg",
 * "topk_select", "k_dict_dfa_match", "k_terms_union_bitmap" (the two regex
 * kernels; other kernels appear under their own names once launched). */
int32_t qw_kernel_stats(qw_ctx* ctx, const char* kernel_name,
                        double* total_ms, uint64_t* launches);
void qw_kernel_stats_reset(qw_ctx* ctx);
int32_t qw_ctx_device_sync(qw_ctx* ctx);

/* HBM footprint accounting (SearchPermitProvider memory-budget analog):
 * used = split images + scratch/result buffers + cached hitset bitmaps;
 * budget = configured "hbm_memory_budget" or 97% of device free memory at
 * first use; splits_bytes = resident split images alone. */
int32_t qw_ctx_memory_stats(qw_ctx* ctx, uint64_t* used_bytes,
                            uint64_t* budget_bytes, uint64_t* splits_bytes);

/* Negative/absence term cache counters (leaf.rs:761-827): probes that
 * short-circuited a split (hits), probes over required terms that found no
 * cached absence (misses), and resident keys. Replaces the reference's
 * prometheus-side SplitSearchOutcomeCounters for this cache. */
int32_t qw_absence_cache_stats(qw_ctx* ctx, uint64_t* hits, uint64_t* misses,
                               uint64_t* entries);

/* Top-K pruning counters: out[0] = collecting leaf-split calls that ran with
 * the tile kernel's top-K pruning on, out[1] = those that ran without it
 * (wide records, K > 64, search_after, or config "topk_prune": false),
 * out[2] / out[3] = candidate records emitted / docs matched by the last
 * collecting call. With pruning off the two are equal. */
int32_t qw_topk_stats(qw_ctx* ctx, uint64_t out[4]);

/* One-sync top-K selection counters. A collecting leaf-split call without a
 * search_after cursor lets the device pick the K-boundary bin and compact
 * the survivors behind the tile kernel, so that they arrive with the call's
 * one synchronize (config "topk_onesync": false keeps the host-side pick).
 * out[0] = calls served that way, out[1] = calls whose boundary bin held too
 * many records and fell back to the host refinement loop, out[2] = survivor
 * records of the last one-sync call, out[3] = 1 when that call needed a
 * second copy for survivors beyond the inline ones, else 0. */
int32_t qw_topk_onesync_stats(qw_ctx* ctx, uint64_t out[4]);

/* Library version + build arch, e.g. "quickwit_amd 0.1 gfx950". */
const char* qw_version(void);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* QUICKWIT_AMD_H */
