// ============================================================================
// libquickwit_amd — MI355X-native host orchestration for the Quickwit
// leaf-search hot path (the PRODUCT; C-ABI in include/quickwit_amd.h).
//
// This is the work the reference ships to its rayon pool inside
// leaf_search_single_split (quickwit/quickwit-search/src/leaf.rs:899-959):
// query build (doc_mapper_impl.rs:637 -> tantivy_query_ast.rs:153-374),
// posting decode + boolean combination + BM25 + collection
// (searcher.search at leaf.rs:929, collector.rs:523-594), fast-field
// predicates (range_query.rs:86-158) and aggregations, top-K with the
// reference tie-breaks (top_k_collector.rs, docs/internals/sorting.md:14-26),
// and the cross-split merge (collector.rs:1198, :832-861).
//
// All index arithmetic runs in HIP kernels on gfx950 (kernels.hip, included
// below as one translation unit — no -fgpu-rdc needed). There is NO CPU
// fallback: without a HIP device every search returns QW_ERR_NO_GPU
// (DESIGN.md §1). The CPU restatement lives in oracle/ (test infra only).
// ============================================================================
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

// the plan layer accepts sloppy phrases and multi-token phrase prefixes only
// here: the CPU oracle shares qast.h and has no evaluator for them, so it
// keeps refusing them (defined before the first include that pulls qast.h in)
#define QW_PHRASE_WINDOW 1
// likewise regex queries (PlanNode::REGEX, the regex AST type and the
// field:/re/ literal)
#define QW_REGEX_QUERY 1

#include "../../include/quickwit_amd.h"
#include "fieldnorm.h"
#include "minijson.h"
#include "pb.h"
#include "qagg_format.h"
#include "qast.h"
#include "qsplit.h"
#include "sortkey.h"

// device code: single TU (kernels + host) so no relocatable device link
#include "kernels.hip"

namespace qw {

#define HIP_CHECK(expr)                                                        \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess)                                                  \
            throw std::runtime_error(std::string("HIP error: ") +              \
                                     hipGetErrorString(_e) + " at " #expr);    \
    } while (0)

struct DeviceSplit {
    std::vector<uint8_t> host;  // host copy: term-dict lookups + meta parse
    SplitView view;             // views into `host` (segment 0 for QWA2)
    uint8_t* d_image = nullptr; // full file image resident in HBM
    size_t len = 0;
    uint64_t total_docs = 0;    // across all segments
    // QWA2 multi-segment container (collector.rs:475-594 per-segment
    // collection): one child per segment; child host/view/d_image alias the
    // parent allocation (owns_image=false)
    std::vector<std::unique_ptr<DeviceSplit>> segs;
    bool owns_image = true;
    // per-(field, term) device block-range tables (u32 lo[ntiles] +
    // hi[ntiles]): they depend only on the split's static block structure,
    // so the O(blocks+tiles) host walk (~180 us at 100M docs) and its
    // 300 KB upload happen once per term, not per query
    mutable std::map<std::pair<const void*, int64_t>, uint8_t*> range_cache;
    mutable uint64_t range_cache_bytes = 0;
    void free_range_cache() const {
        for (auto& kv : range_cache) (void)hipFree(kv.second);
        range_cache.clear();
        range_cache_bytes = 0;
    }
};

struct KernelTimer {
    double total_ms = 0;
    uint64_t launches = 0;
};

struct DevBuf {  // grow-only device scratch
    uint8_t* p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        HIP_CHECK(hipMalloc(&p, n));
        cap = n;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct PinnedBuf {  // grow-only pinned host staging (fast H2D/D2H, no
                    // per-call allocation)
    uint8_t* p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        HIP_CHECK(hipHostMalloc((void**)&p, n));
        cap = n;
    }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// LeafSearchCache restatement (quickwit-search/src/leaf_cache.rs): memoizes
// per-(split, canonical request) LeafSearchResponse bytes in a byte-capacity
// LRU (MemorySizedCache semantics). The key canonicalizes the request by
// clearing the timestamp bounds and forcing count_hits = COUNT_ALL
// (leaf_cache.rs:86-115) and appends the merged (request ∩ split) half-open
// time range (leaf_cache.rs:118-180).
struct LeafCache {
    size_t capacity = 64ull << 20;  // SearcherConfig partial_request_cache_capacity
    size_t used = 0;
    std::list<std::pair<std::string, std::string>> lru;  // front = most recent
    std::map<std::string, std::list<std::pair<std::string, std::string>>::iterator> idx;

    bool get(const std::string& key, std::string* out) {
        auto it = idx.find(key);
        if (it == idx.end()) return false;
        lru.splice(lru.begin(), lru, it->second);
        *out = it->second->second;
        return true;
    }
    void put(const std::string& key, std::string val) {
        if (!capacity || key.size() + val.size() > capacity) return;
        auto it = idx.find(key);
        if (it != idx.end()) {
            used -= it->second->first.size() + it->second->second.size();
            lru.erase(it->second);
            idx.erase(it);
        }
        used += key.size() + val.size();
        lru.emplace_front(key, std::move(val));
        idx[key] = lru.begin();
        while (used > capacity && !lru.empty()) {
            auto& back = lru.back();
            used -= back.first.size() + back.second.size();
            idx.erase(back.first);
            lru.pop_back();
        }
    }
    void remove_split(const std::string& split_id) {
        std::string prefix = split_id + '\0';
        for (auto it = lru.begin(); it != lru.end();) {
            if (it->first.compare(0, prefix.size(), prefix) == 0) {
                used -= it->first.size() + it->second.size();
                idx.erase(it->first);
                it = lru.erase(it);
            } else ++it;
        }
    }
};

// half-open [start, end) second range; has_end=false means unbounded
// (leaf_cache.rs HalfOpenRange, incl. the empty-range normalization)
struct HalfOpen {
    int64_t start = INT64_MIN;
    bool has_end = false;
    int64_t end = 0;
    void normalize() {
        if (has_end && end <= start) {
            start = 0;
            end = 0;
            has_end = true;
        }
    }
};

static std::string leaf_cache_key(const pb::SplitIdAndFooterOffsets& so,
                                  const pb::SearchRequest& req) {
    // request time range: [start included, end excluded)
    HalfOpen r;
    r.start = req.start_timestamp ? *req.start_timestamp : INT64_MIN;
    if (req.end_timestamp) {
        r.has_end = true;
        r.end = *req.end_timestamp;
    }
    r.normalize();
    // split time range: [start, end] inclusive -> [start, end+1)
    HalfOpen s;
    s.start = so.timestamp_start ? *so.timestamp_start : INT64_MIN;
    if (so.timestamp_end && *so.timestamp_end != INT64_MAX) {
        s.has_end = true;
        s.end = *so.timestamp_end + 1;
    }
    s.normalize();
    // intersection
    HalfOpen m;
    m.start = std::max(r.start, s.start);
    if (r.has_end || s.has_end) {
        m.has_end = true;
        m.end = r.has_end && s.has_end ? std::min(r.end, s.end)
                                       : (r.has_end ? r.end : s.end);
    }
    m.normalize();
    pb::SearchRequest canon = req;
    canon.start_timestamp.reset();
    canon.end_timestamp.reset();
    canon.count_hits = 0;  // CountHits::CountAll (leaf_cache.rs:108)
    std::string key = so.split_id;
    key += '\0';
    char rng[17];
    memcpy(rng, &m.start, 8);
    memcpy(rng + 8, &m.end, 8);
    rng[16] = m.has_end ? 1 : 0;
    key.append(rng, 17);
    key += canon.encode();
    return key;
}

// device HitSet bitmaps memoized per (split, subquery fingerprint) — the
// MI355X-native PredicateCache (cache_node.rs:202-486).
// Count-capped LRU; a 100M-doc bitmap is 12.5 MB of HBM.
struct HitsetCache {
    // Count-capped LRU of device bitmaps. Entries touched by the CURRENT
    // query (gen == cur_gen) are pinned: resolve_hitset/bitmap_eval return
    // raw device pointers that the later main-kernel launch reads, so an
    // eviction between resolve and launch would free in-use device memory.
    // begin_query() unpins everything from previous queries.
    struct Entry {
        std::string key;
        uint8_t* bm;
        uint64_t gen;
        uint64_t size;
    };
    size_t cap = 256;
    uint64_t cur_gen = 0;
    uint64_t bytes = 0;  // device bytes held (feeds the ctx HBM accounting)
    std::list<Entry> lru;
    std::map<std::string, std::list<Entry>::iterator> idx;
    uint64_t hits = 0, misses = 0;

    void begin_query() { ++cur_gen; }
    uint8_t* get(const std::string& key) {
        auto it = idx.find(key);
        if (it == idx.end()) {
            ++misses;
            return nullptr;
        }
        ++hits;
        it->second->gen = cur_gen;
        lru.splice(lru.begin(), lru, it->second);
        return it->second->bm;
    }
    void put(const std::string& key, uint8_t* bm, uint64_t size) {
        lru.push_front(Entry{key, bm, cur_gen, size});
        idx[key] = lru.begin();
        bytes += size;
        // evict oldest UNPINNED entries; a query resolving > cap distinct
        // subtrees temporarily overflows the cap rather than freeing memory
        // the pending launch still references
        for (auto it = std::prev(lru.end());
             lru.size() > cap && it != lru.begin();) {
            auto cur = it--;
            if (cur->gen == cur_gen) continue;
            (void)hipFree(cur->bm);
            bytes -= cur->size;
            idx.erase(cur->key);
            lru.erase(cur);
        }
    }
    void remove_split(const std::string& split_id) {
        std::string prefix = split_id + '\0';
        for (auto it = lru.begin(); it != lru.end();) {
            if (it->key.compare(0, prefix.size(), prefix) == 0) {
                (void)hipFree(it->bm);
                bytes -= it->size;
                idx.erase(it->key);
                it = lru.erase(it);
            } else ++it;
        }
    }
    void clear() {
        for (auto& e : lru) (void)hipFree(e.bm);
        lru.clear();
        idx.clear();
        bytes = 0;
    }
};

}  // namespace qw

// negative/absence term cache (leaf.rs:761-827): (split, field, term) keys
// proven absent from the split's term dictionary by an earlier search; a
// probe hit short-circuits the whole split search (the reference aborts
// during warmup, leaf.rs:315-320 / 472-477; key analog of
// term_absence_cache_key, leaf.rs:641-652)
struct AbsenceCache {
    std::set<std::string> keys;
    uint64_t hits = 0, misses = 0;
    size_t cap = 1 << 20;
    static std::string key(const std::string& split_id, const std::string& f,
                           const std::string& t) {
        std::string k = split_id;
        k += '\0';
        k += f;
        k += '\x1f';
        k += t;
        return k;
    }
    void remove_split(const std::string& split_id) {
        std::string lo = split_id + '\0';
        std::string hi = split_id + '\x01';
        keys.erase(keys.lower_bound(lo), keys.lower_bound(hi));
    }
};

struct qw_ctx {
    int device = 0;
    bool device_ready = false;
    int64_t agg_bucket_limit = 65000;
    std::map<std::string, std::unique_ptr<qw::DeviceSplit>> splits;
    qw::LeafCache leaf_cache;
    qw::HitsetCache hitsets;
    AbsenceCache absence;
    std::string last_error;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    qw::DevBuf d_scratch, d_results, d_survivors, d_cand2;
    qw::PinnedBuf h_scratch, h_counts, h_surv, h_topk, h_agg;  // pinned staging
    std::map<std::string, qw::KernelTimer> timers;
    // HBM accounting (SearchPermitProvider memory-budget analog,
    // search_permit_provider.rs:43-110): split images + scratch/result
    // buffers in hbm_used, hitset bitmaps in hitsets.bytes. budget 0 =
    // resolved from device free memory at first use; config key
    // "hbm_memory_budget" overrides (bytes). Over-budget add_split refuses
    // (QW_ERR_OVER_MEMORY_BUDGET); over-budget search scratch fails that
    // split into failed_splits, like a permit that can never be granted.
    uint64_t hbm_used = 0;
    uint64_t hbm_budget = 0;
    bool budget_configured = false;
    // top-K pruning in the tile kernel; config key
    // "topk_prune" (bool, default true) turns it off for this context, so
    // one process can hold a pruned and an unpruned searcher. Counters for
    // qw_topk_stats: collecting leaf calls pruned / unpruned, and the last
    // collecting call's emitted candidates and matched docs.
    bool topk_prune = true;
    uint64_t topk_pruned = 0, topk_unpruned = 0;
    uint64_t topk_last_emitted = 0, topk_last_matched = 0;
    // one-sync top-K selection (TopkSelector); config key "topk_onesync"
    // (bool, default true) turns it off for this context. Counters for
    // qw_topk_onesync_stats: collecting calls whose survivors came with the
    // main synchronize / that fell back to the host refinement loop, and
    // the last one-sync call's survivor count and whether it needed the
    // second copy.
    bool topk_onesync = true;
    uint64_t topk_onesync_calls = 0, topk_onesync_fallbacks = 0;
    uint64_t topk_onesync_last_survivors = 0, topk_onesync_last_tail = 0;
};

static void qw_check_budget(qw_ctx* ctx, uint64_t need) {
    uint64_t used = ctx->hbm_used + ctx->hitsets.bytes;
    if (ctx->hbm_budget && used + need > ctx->hbm_budget)
        throw std::runtime_error(
            "HBM memory budget exceeded: used " + std::to_string(used) +
            " + need " + std::to_string(need) + " > budget " +
            std::to_string(ctx->hbm_budget) +
            " (search_permit_provider analog; raise hbm_memory_budget or "
            "remove splits)");
}

// budgeted grow of a ctx scratch DevBuf
static void qw_ensure_acct(qw_ctx* ctx, qw::DevBuf& b, size_t n) {
    if (n <= b.cap) return;
    qw_check_budget(ctx, n - b.cap);
    ctx->hbm_used -= b.cap;
    b.ensure(n);
    ctx->hbm_used += b.cap;
}

// device address of the (split, term) block-range table, computed and
// uploaded on first use (DeviceSplit::range_cache)
static uint64_t term_ranges_addr(qw_ctx* ctx, const qw::DeviceSplit& ds,
                                 const qw::TextFieldView* f, int64_t tid,
                                 uint32_t n_tiles, uint32_t num_docs) {
    using namespace qw;
    auto key = std::make_pair((const void*)f, tid);
    auto it = ds.range_cache.find(key);
    if (it != ds.range_cache.end()) return (uint64_t)it->second;
    if (ds.range_cache.size() >= 1024) {  // wildcard-expansion backstop
        ctx->hbm_used -= ds.range_cache_bytes;
        ds.free_range_cache();
    }
    size_t bytes = 2ull * n_tiles * 4;
    qw_check_budget(ctx, bytes);
    std::vector<uint32_t> r(2ull * n_tiles);
    const SkipEntry* sk = f->h_skip + f->h_skip_off[tid] / 16;
    uint32_t nb = f->h_n_blocks[tid];
    uint32_t* lo = r.data();
    uint32_t* hi = lo + n_tiles;
    uint32_t b_lo = 0, b_hi = 0;
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
        uint32_t tlo = tile * TILE_DOCS;
        uint32_t thi = std::min<uint32_t>(tlo + TILE_DOCS, num_docs);
        while (b_lo < nb && sk[b_lo].last_doc < tlo) ++b_lo;
        if (b_hi < b_lo) b_hi = b_lo;
        while (b_hi < nb && sk[b_hi].first_doc < thi) ++b_hi;
        lo[tile] = b_lo;
        hi[tile] = b_hi;
    }
    uint8_t* d = nullptr;
    HIP_CHECK(hipMalloc(&d, bytes));
    HIP_CHECK(hipMemcpy(d, r.data(), bytes, hipMemcpyHostToDevice));
    ctx->hbm_used += bytes;
    ds.range_cache.emplace(key, d);
    ds.range_cache_bytes += bytes;
    return (uint64_t)d;
}

static void ctx_ensure_device(qw_ctx* ctx) {
    using namespace qw;
    if (ctx->device_ready) return;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        throw std::runtime_error("no HIP device visible");
    if (ctx->device >= n) throw std::runtime_error("bad device ordinal");
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&ctx->ev_start));
    HIP_CHECK(hipEventCreate(&ctx->ev_stop));
    if (!ctx->budget_configured) {
        // default budget: 97% of the device's free HBM at first use
        // (warmup_memory_budget analog, node_config defaults)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b)
            ctx->hbm_budget = uint64_t(free_b) / 100 * 97;
    }
    ctx->device_ready = true;
}

namespace qw {

// ------------------------------------------------------------ flattening
// The kernel executes ONE flattened boolean level (should/must/must_not term
// lists + fast-field predicates). This covers every BASELINE.json config and
// the golden-suite query shapes (term, full_text and/or, bool with
// term/range clauses, range, match_all). A plan that does not flatten throws
// NotFlattenable and is answered from device bitmaps instead
// (flatten_or_bitmap): unscored, the whole tree becomes one PRED_BITSET;
// scored, scored_tree_plan turns its term leaves into gated should terms
// (DESIGN.md §7a). What neither route computes exactly is refused with
// InvalidQuery — never silently mis-answered.
struct NotFlattenable : std::runtime_error {
    // TREE: a boolean shape; with or without scores the bitmap routes answer
    // it. BITMAP: phrase / regex, which have a match set but no score.
    enum Why { TREE, BITMAP } why;
    NotFlattenable(Why w, const char* msg) : std::runtime_error(msg), why(w) {}
};

struct FlatQuery {
    bool match_none = false;
    bool match_all = false;  // positive base = all docs (preds still filter)
    bool scoring = false;
    uint32_t msm = 0;  // >0: shoulds required (count >= msm)
    // required (must/filter) single terms proven ABSENT from this split's
    // term dict during flattening — feeds the negative term cache
    // (leaf.rs:761-827 / term_absence_cache_key leaf.rs:641-652)
    std::vector<std::pair<std::string, std::string>> absent_required;
    struct FTerm {
        const TextFieldView* f;
        int64_t tid;
        uint32_t role;
        float weight;  // BM25 W (0 for unscored filter terms)
        uint32_t grp = 0;  // must-group (OR within a group, AND across)
    };
    std::vector<FTerm> terms;
    uint32_t n_must_groups = 0;
    // CACHE nodes in filter position: resolved to device HitSet bitmaps
    // (PRED_BITSET) by the caller (predicate cache)
    std::vector<const PlanNode*> cache_nodes;
    std::vector<PredDev> preds;
    std::vector<const TextFieldView*> ktab_fields;  // ktab_idx -> field
    // scored tree plans: per term, the device VA of its gate bitmap (0 =
    // ungated term). Empty = no term is gated, the plain tile kernel runs.
    std::vector<uint64_t> gates;

    uint32_t ktab_for(const TextFieldView* f) {
        for (size_t i = 0; i < ktab_fields.size(); ++i)
            if (ktab_fields[i] == f) return uint32_t(i);
        ktab_fields.push_back(f);
        return uint32_t(ktab_fields.size() - 1);
    }
};

static std::string fold_lower(const std::string& s) {
    std::string o = s;
    for (char& c : o) c = char(std::tolower((unsigned char)c));
    return o;
}

static float bm25_weight(const SplitView& sv, const TextFieldView& f, int64_t tid,
                         float boost) {
    double N = double(sv.num_docs);
    double df = double(f.h_doc_freq[tid]);
    double idf = std::log(1.0 + (N - df + 0.5) / (df + 0.5));
    return float(idf * (1.0 + 1.2) * double(boost));
}

static void add_range_pred(FlatQuery& fq, const SplitView& sv, const PlanNode& n,
                           bool negated) {
    const FastFieldView* f = sv.fast_field(n.field);
    PredDev p{};
    if (!f && n.kind == PlanNode::FIELD_PRESENCE) {
        // presence over a text-only field: a doc has the field iff its
        // fieldnorm byte is nonzero (>= 1 token; index_field_presence analog)
        const TextFieldView* tf = sv.text_field(n.field);
        if (tf && tf->has_norms) {
            p.type = PRED_RANGE_U64;
            p.flags = (negated ? PRED_NEGATED : 0) | PRED_LO_INCLUDED;
            p.lo = 1;
            p.values_off = tf->fieldnorms.off;
            p.value_width = 1;
            fq.preds.push_back(p);
            return;
        }
    }
    if (!f) {
        // unknown fast field: matches nothing (oracle eval_range -> empty)
        if (negated) return;  // must_not nothing = no-op
        fq.match_none = true;
        return;
    }
    if (f->type == FastFieldView::MIXED && n.kind != PlanNode::FIELD_PRESENCE)
        throw std::runtime_error(
            "range/term over a mixed-type dynamic column (r2 limit: sorting "
            "and search_after are supported; typed predicates are not)");
    p.type = f->type == FastFieldView::U64   ? PRED_RANGE_U64
             : f->type == FastFieldView::F64 ? PRED_RANGE_F64
                                             : PRED_RANGE_I64;
    p.flags = negated ? PRED_NEGATED : 0;
    if (n.kind == PlanNode::FIELD_PRESENCE) {
        if (!f->nullable && !f->multi && !negated) return;  // always present
        if (!f->nullable && !f->multi && negated) {
            fq.match_none = true;
            return;
        }
        p.type = PRED_PRESENCE;
        if (f->multi) p.offsets_off = f->value_offsets.off;
    } else {
        if (n.lo.kind == Bound::INCLUDED) p.flags |= PRED_LO_INCLUDED;
        if (n.lo.kind == Bound::EXCLUDED) p.flags |= PRED_LO_EXCLUDED;
        if (n.hi.kind == Bound::INCLUDED) p.flags |= PRED_HI_INCLUDED;
        if (n.hi.kind == Bound::EXCLUDED) p.flags |= PRED_HI_EXCLUDED;
        if (f->type == FastFieldView::F64) {
            memcpy(&p.lo, &n.lo.fval, 8);  // bit-cast double bounds
            memcpy(&p.hi, &n.hi.fval, 8);
        } else if (f->type == FastFieldView::STR) {
            // lexicographic bounds -> ord space [lo, hi) over the sorted
            // dict; a lowercase-normalized column folds the bounds too;
            // multi-valued columns match when ANY value is in range
            if (f->multi) p.offsets_off = f->value_offsets.off;
            std::string lo_s = f->lower_norm ? fold_lower(n.lo.sval) : n.lo.sval;
            std::string hi_s = f->lower_norm ? fold_lower(n.hi.sval) : n.hi.sval;
            p.type = PRED_RANGE_U64;
            p.flags &= PRED_NEGATED;  // rebuild the bound flags below
            if (n.lo.kind != Bound::UNBOUNDED) {
                p.flags |= PRED_LO_INCLUDED;
                p.lo = int64_t(
                    f->str_bound_ord(lo_s, n.lo.kind == Bound::EXCLUDED));
            }
            if (n.hi.kind != Bound::UNBOUNDED) {
                p.flags |= PRED_HI_EXCLUDED;
                p.hi = int64_t(
                    f->str_bound_ord(hi_s, n.hi.kind == Bound::INCLUDED));
            }
        } else {
            p.lo = n.lo.ival;
            p.hi = n.hi.ival;
        }
    }
    p.values_off = f->values.off;
    p.nulls_off = f->nullable ? f->nulls.off : 0;
    p.value_width = f->type == FastFieldView::STR ? uint32_t(f->ord_width) : 8;
    fq.preds.push_back(p);
}

static void add_term(FlatQuery& fq, const SplitView& sv, const std::string& field,
                     const std::string& value, uint32_t role, float boost,
                     bool scored, uint32_t grp = 0, bool group_member = false) {
    const TextFieldView* f = sv.text_field(field);
    int64_t tid = f ? f->find_term(value.data(), value.size()) : -1;
    if (tid < 0) {
        // absent term: MUST -> split matches nothing; SHOULD/MUST_NOT -> skip
        // (skipped shoulds can never satisfy msm — handled by caller count).
        // A member of a must OR-GROUP only weakens the group when absent.
        if (role == ROLE_MUST && !group_member) {
            fq.match_none = true;
            fq.absent_required.emplace_back(field, value);
        }
        return;
    }
    FlatQuery::FTerm t;
    t.f = f;
    t.tid = tid;
    t.role = role;
    t.weight = scored ? bm25_weight(sv, *f, tid, boost) : 0.f;
    t.grp = grp;
    fq.terms.push_back(t);
}

// expand a wildcard over the field's term dictionary (qast.h glob_match;
// wildcard_query.rs -> AutomatonQuery). Returns the number of matched terms.
static size_t add_wildcard(FlatQuery& fq, const SplitView& sv, const PlanNode& n,
                           uint32_t role, uint32_t grp) {
    const TextFieldView* f = sv.text_field(n.field);
    if (!f) return 0;
    size_t cnt = 0;
    for (uint32_t t = 0; t < f->num_terms; ++t) {
        const char* s = (const char*)f->h_term_bytes + f->h_term_offsets[t];
        size_t sl = f->h_term_offsets[t + 1] - f->h_term_offsets[t];
        if (!glob_match(s, sl, n.value.data(), n.value.size(), n.ci)) continue;
        FlatQuery::FTerm ft;
        ft.f = f;
        ft.tid = t;
        ft.role = role;
        ft.weight = 0.f;  // const-score node; scored plans were rejected
        ft.grp = grp;
        fq.terms.push_back(ft);
        if (++cnt > 4096)
            throw std::runtime_error("wildcard expands to >4096 terms (GPU r1 limit)");
    }
    return cnt;
}

// strip semantics-transparent cache wrappers (contexts that cannot use the
// bitmap: should/must_not/scored root)
static const PlanNode& uncache(const PlanNode& c) {
    return c.kind == PlanNode::CACHE ? uncache(c.cache_inner.front()) : c;
}

static bool is_pure_should_terms(const PlanNode& n) {
    if (n.kind != PlanNode::BOOL) return false;
    if (!n.must.empty() || !n.must_not.empty() || !n.filter.empty()) return false;
    if (n.minimum_should_match > 1) return false;
    for (auto& c : n.should)
        if (c.kind != PlanNode::TERM) return false;
    return true;
}

static bool is_pure_must_terms(const PlanNode& n) {
    if (n.kind != PlanNode::BOOL) return false;
    if (!n.should.empty() || !n.must_not.empty() || !n.filter.empty()) return false;
    for (auto& c : n.must)
        if (c.kind != PlanNode::TERM) return false;
    return true;
}

static void add_positive(FlatQuery& fq, const SplitView& sv, const PlanNode& c,
                         bool scored, float boost);

static void flatten_bool(FlatQuery& fq, const SplitView& sv, const PlanNode& n,
                         float boost);

// a MUST/FILTER clause
static void add_positive(FlatQuery& fq, const SplitView& sv, const PlanNode& c,
                         bool scored, float boost) {
    switch (c.kind) {
        case PlanNode::CACHE:
            fq.cache_nodes.push_back(&c);
            break;
        case PlanNode::TERM:
            add_term(fq, sv, c.field, c.value, ROLE_MUST, boost * c.boost, scored,
                     fq.n_must_groups++);
            break;
        case PlanNode::WILDCARD:
            if (add_wildcard(fq, sv, c, ROLE_MUST, fq.n_must_groups++) == 0)
                fq.match_none = true;  // must clause matching nothing
            break;
        case PlanNode::RANGE:
        case PlanNode::FIELD_PRESENCE:
            add_range_pred(fq, sv, c, false);
            break;
        case PlanNode::MATCH_ALL:
            break;  // no constraint
        case PlanNode::MATCH_NONE:
            fq.match_none = true;
            break;
        case PlanNode::BOOL:
            if (is_pure_must_terms(c)) {
                for (auto& m : c.must)
                    add_term(fq, sv, m.field, m.value, ROLE_MUST,
                             boost * c.boost * m.boost, scored,
                             fq.n_must_groups++);
            } else if (is_pure_should_terms(c)) {
                // OR-of-terms under must/filter: one must-GROUP (the kernel
                // ORs the group's bitsets, then ANDs the groups)
                uint32_t grp = fq.n_must_groups++;
                size_t before = fq.terms.size();
                for (auto& s : c.should)
                    add_term(fq, sv, s.field, s.value, ROLE_MUST,
                             boost * c.boost * s.boost, scored, grp, true);
                if (fq.terms.size() == before) fq.match_none = true;
            } else {
                throw NotFlattenable(
                    NotFlattenable::TREE,
                    "nested boolean inside must/filter not flattenable (GPU r1)");
            }
            break;
        case PlanNode::PHRASE:
            throw NotFlattenable(
                NotFlattenable::BITMAP,
                "phrase clause not flattenable (device-bitmap path)");
        case PlanNode::REGEX:
            throw NotFlattenable(
                NotFlattenable::BITMAP,
                "regex clause not flattenable (device-bitmap path)");
    }
}

static void flatten_bool(FlatQuery& fq, const SplitView& sv, const PlanNode& n,
                         float boost) {
    boost *= n.boost;
    if (n.must.empty() && n.filter.empty() && n.should.empty() &&
        n.must_not.empty() && n.minimum_should_match <= 0) {
        // empty bool is match_all by ES convention (tantivy_query_ast.rs:193)
        fq.match_all = true;
        return;
    }
    bool has_req = !n.must.empty() || !n.filter.empty();
    for (auto& c : n.must) add_positive(fq, sv, c, fq.scoring, boost);
    for (auto& c : n.filter) add_positive(fq, sv, c, false, boost);

    // shoulds: flatten TERM / pure-OR bool children into SHOULD terms
    size_t should_clauses = 0;
    for (auto& c_raw : n.should) {
        const PlanNode& c = uncache(c_raw);
        if (c.kind == PlanNode::TERM) {
            add_term(fq, sv, c.field, c.value, ROLE_SHOULD, boost * c.boost,
                     fq.scoring);
            ++should_clauses;
        } else if (is_pure_should_terms(c)) {
            // OR-of-terms child: each term is an independent SHOULD here; one
            // clause satisfied iff any term matches — valid for msm<=1 only
            for (auto& t : c.should)
                add_term(fq, sv, t.field, t.value, ROLE_SHOULD,
                         boost * c.boost * t.boost, fq.scoring);
            ++should_clauses;
        } else if (c.kind == PlanNode::WILDCARD) {
            add_wildcard(fq, sv, c, ROLE_SHOULD, 0);
            ++should_clauses;
        } else if (c.kind == PlanNode::MATCH_NONE) {
            // contributes nothing
        } else {
            throw NotFlattenable(NotFlattenable::TREE,
                                 "should clause not flattenable (GPU r1)");
        }
    }

    for (auto& c_raw : n.must_not) {
        const PlanNode& c = uncache(c_raw);
        if (c.kind == PlanNode::TERM)
            add_term(fq, sv, c.field, c.value, ROLE_MUST_NOT, 1.f, false);
        else if (c.kind == PlanNode::RANGE || c.kind == PlanNode::FIELD_PRESENCE)
            add_range_pred(fq, sv, c, true);
        else if (c.kind == PlanNode::WILDCARD)
            add_wildcard(fq, sv, c, ROLE_MUST_NOT, 0);
        else if (is_pure_should_terms(c))
            // not(a or b) = not a and not b: must_not is a union-then-subtract
            for (auto& t : c.should)
                add_term(fq, sv, t.field, t.value, ROLE_MUST_NOT, 1.f, false);
        else if (c.kind == PlanNode::MATCH_NONE) {
        } else if (c.kind == PlanNode::MATCH_ALL) {
            fq.match_none = true;
        } else
            throw NotFlattenable(NotFlattenable::TREE,
                                 "must_not clause not flattenable (GPU r1)");
    }

    int64_t msm = n.minimum_should_match;
    // unset OR non-positive: shoulds are optional beside musts, but with no
    // positive clause at least one should must match (bool_query.rs:34-45 —
    // the es_compat msm=0/negative cases pin this)
    if (msm <= 0) msm = has_req ? 0 : 1;
    bool nested_or = false;
    for (auto& c : n.should) nested_or |= c.kind != PlanNode::TERM;
    if (msm > 1 && nested_or)
        throw std::runtime_error("minimum_should_match>1 over nested clauses");
    if (should_clauses == 0 && msm > 0 && !n.should.empty()) {
        fq.match_none = true;  // all required shoulds were absent terms
        return;
    }
    if (!has_req && n.should.empty()) {
        if (n.must_not.empty()) {
            fq.match_none = true;  // no clause at all matches nothing
            return;
        }
        // must_not only: implicit match_all base
        // (tantivy_query_ast.rs:310-322 pushes match_all)
        fq.match_all = true;
        fq.msm = 0;
        return;
    }
    fq.msm = uint32_t(msm);
    uint32_t n_must_terms = 0, n_should_terms = 0;
    for (auto& t : fq.terms) {
        n_must_terms += t.role == ROLE_MUST;
        n_should_terms += t.role == ROLE_SHOULD;
    }
    if (msm > 0 && n_should_terms == 0) {
        fq.match_none = true;  // required shoulds but every term absent
        return;
    }
    // the tile kernel's scored match test is "score > 0", which is msm == 1
    // over the shoulds alone; scored_tree_plan answers the other two forms
    if (fq.scoring && msm > 0 && n_must_terms > 0)
        throw NotFlattenable(
            NotFlattenable::TREE,
            "scored msm>0 with must terms not supported (GPU r1)");
    if (fq.scoring && msm > 1)
        throw NotFlattenable(
            NotFlattenable::TREE,
            "scored minimum_should_match>1 not supported (GPU r1)");
    // base: match_all when no must terms (pred-only/should-optional base)
    fq.match_all = n_must_terms == 0 && (has_req || msm == 0);
    if (!has_req && msm == 0 && n.should.empty()) fq.match_none = true;
}

static FlatQuery flatten(const SplitView& sv, const PlanNode& plan, bool scoring) {
    FlatQuery fq;
    fq.scoring = scoring;
    if (scoring && plan_has_const_score(plan))
        throw std::runtime_error(
            "term_set/wildcard/phrase/regex under _score sorting not supported "
            "(const-score semantics, qast.h)");
    if (plan.kind == PlanNode::PHRASE)
        throw NotFlattenable(NotFlattenable::BITMAP,
                             "phrase not flattenable (device-bitmap path)");
    if (plan.kind == PlanNode::REGEX)
        throw NotFlattenable(NotFlattenable::BITMAP,
                             "regex not flattenable (device-bitmap path)");
    switch (plan.kind) {
        case PlanNode::MATCH_ALL:
            fq.match_all = true;
            break;
        case PlanNode::MATCH_NONE:
            fq.match_none = true;
            break;
        case PlanNode::TERM:
            add_term(fq, sv, plan.field, plan.value, ROLE_SHOULD, plan.boost, scoring);
            if (fq.terms.empty()) fq.match_none = true;
            fq.msm = 1;
            break;
        case PlanNode::RANGE:
        case PlanNode::FIELD_PRESENCE:
            fq.match_all = true;
            add_range_pred(fq, sv, plan, false);
            break;
        case PlanNode::WILDCARD:
            add_wildcard(fq, sv, plan, ROLE_SHOULD, 0);
            if (fq.terms.empty()) fq.match_none = true;
            fq.msm = 1;
            break;
        case PlanNode::CACHE:
            if (!scoring) {  // root cache: match_all base + cached bitmap
                fq.match_all = true;
                fq.cache_nodes.push_back(&plan);
            } else {
                return flatten(sv, uncache(plan), scoring);
            }
            break;
        case PlanNode::BOOL:
            flatten_bool(fq, sv, plan, 1.f);
            break;
    }
    if (fq.scoring)
        for (auto& t : fq.terms)
            if (t.role == ROLE_SHOULD && fq.msm > 0 && t.weight <= 0.f)
                throw std::runtime_error("non-positive BM25 weight (boost<=0?)");
    return fq;
}

// ------------------------------------------------------------ agg planning
struct AggPlan {
    std::vector<AggDef> defs;
    std::vector<AggDev> devs;            // one per def
    std::vector<const FastFieldView*> fields;
    // composite aggs: per-source column views (null for other kinds)
    std::vector<std::array<const FastFieldView*, 4>> comp_fields;
    // composite aggs: per-source bit widths of the packed key (decode reads
    // these back instead of re-deriving them)
    std::vector<std::array<uint32_t, 4>> comp_width;
    // percentiles: per-agg gamma^k boundary doubles (appended to scratch;
    // empty for aggs without a sketch)
    std::vector<std::vector<double>> pbounds;
    size_t out_bytes = 0;                // total result bytes (counts + subs)
    std::vector<uint8_t> init;           // initial contents of the out region
};

static void col_min_max(const FastFieldView& f, double* mn, double* mx) {
    if (f.type == FastFieldView::U64) {
        *mn = double(uint64_t(f.min_value));
        *mx = double(uint64_t(f.max_value));
    } else if (f.type == FastFieldView::F64) {
        *mn = f.fmin;
        *mx = f.fmax;
    } else {
        *mn = double(f.min_value);
        *mx = double(f.max_value);
    }
}

static AggPlan plan_aggs(const SplitView& sv, const std::string& agg_json,
                         int64_t bucket_limit, uint64_t out_base) {
    AggPlan ap;
    ap.defs = parse_agg_request(agg_json);
    {
        auto agg_col_type = [&](const std::string& name) -> int {
            const FastFieldView* cf = sv.fast_field(name);
            return cf ? int(cf->type) : -1;
        };
        validate_agg_fields(ap.defs, agg_col_type);
    }
    uint64_t off = out_base;
    for (const AggDef& d : ap.defs) {
        const FastFieldView* f = sv.fast_field(d.field);
        ap.fields.push_back(f);
        ap.comp_fields.push_back({nullptr, nullptr, nullptr, nullptr});
        ap.comp_width.push_back({0, 0, 0, 0});
        ap.pbounds.emplace_back();
        AggDev a{};
        a.lds_slot = 0xFF;
        a.p_si = 0xFF;
        if (d.kind == AggDef::COMPOSITE) {
            a.kind = AGGD_COMP;
            bool all_present = true;
            for (const CompSource& cs : d.comp) {
                const FastFieldView* sf = sv.fast_field(cs.field);
                if (!sf) { all_present = false; continue; }
                if (!cs.is_histo && sf->type != FastFieldView::STR)
                    throw std::runtime_error(
                        "composite terms source over a numeric column "
                        "(r1 limit)");
                if (cs.is_histo && sf->type == FastFieldView::STR)
                    throw std::runtime_error(
                        "composite histogram source over a str column");
                if (sf->multi)
                    throw std::runtime_error(
                        "composite source over a multi-valued column "
                        "(r1 limit)");
            }
            if (all_present) {
                if (sv.num_docs > (1u << 21))
                    throw std::runtime_error(
                        "composite aggregation on a >2M-doc split (r1 limit)");
                // pack sources MSB-first; component value count per source
                // bounds its bit width (comp_key_bits in qagg_format.h keeps
                // assembly decode in lockstep)
                uint32_t acc = 0;
                for (int si = int(d.comp.size()) - 1; si >= 0; --si) {
                    const CompSource& cs = d.comp[si];
                    const FastFieldView* sf = sv.fast_field(cs.field);
                    ap.comp_fields.back()[si] = sf;
                    uint64_t miss = cs.missing_bucket ? 1 : 0;
                    uint64_t n_values;
                    if (cs.is_histo) {
                        double mn, mx;
                        col_min_max(*sf, &mn, &mx);
                        int64_t b0 = int64_t(
                            std::floor((mn - cs.offset) / cs.interval));
                        int64_t b1 = int64_t(
                            std::floor((mx - cs.offset) / cs.interval));
                        a.c_base[si] = b0;
                        a.c_interval[si] = cs.interval;
                        a.c_offset[si] = cs.offset;
                        a.c_histo |= 1u << si;
                        n_values = uint64_t(b1 - b0 + 1) + miss;
                    } else {
                        n_values = uint64_t(sf->cardinality) + miss;
                    }
                    if (miss) a.c_missing |= 1u << si;
                    a.sub_values_off[si] = sf->values.off;
                    a.sub_nulls_off[si] = sf->nullable ? sf->nulls.off : 0;
                    a.sub_width[si] = cs.is_histo ? 8 : uint32_t(sf->ord_width);
                    a.sub_is_i64[si] =
                        sf->type == FastFieldView::U64   ? 0
                        : sf->type == FastFieldView::F64 ? 2
                                                         : 1;
                    a.c_shift[si] = acc;
                    ap.comp_width.back()[si] = comp_key_bits(n_values);
                    acc += ap.comp_width.back()[si];
                }
                if (acc > 63)
                    throw std::runtime_error(
                        "composite key exceeds 63 bits (r1 limit)");
                a.n_sub = uint32_t(d.comp.size());
                uint64_t want = uint64_t(sv.num_docs) * 2;
                uint32_t slots = 1024;
                while (slots < want) slots <<= 1;
                a.n_buckets = slots * 2 + 2;
            } else {
                a.n_buckets = 0;  // a source column is absent: empty result
            }
        } else if (d.kind == AggDef::TERMS || d.kind == AggDef::CARDINALITY) {
            a.kind = AGGD_TERMS;
            if (d.kind == AggDef::TERMS) {
                // a percentiles sub has no value to order by: the refusal
                // terms_order_sub_value would give at truncation, for every
                // split and whatever its term count
                std::string oname = d.order_target, ostat;
                size_t dot = d.order_target.rfind('.');
                if (dot != std::string::npos) {
                    oname = d.order_target.substr(0, dot);
                    ostat = d.order_target.substr(dot + 1);
                }
                for (auto& s : d.sub)
                    if (s.kind == MetricAgg::PERCENTILES &&
                        (s.name == oname || s.name == d.order_target))
                        throw std::runtime_error("terms order: unknown stat '" +
                                                 ostat + "'");
            }
            if (f && f->type == FastFieldView::STR) {
                a.n_buckets = f->cardinality;
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = uint32_t(f->ord_width);
                if (f->multi) a.offsets_off = f->value_offsets.off;
                if (d.kind == AggDef::TERMS && !d.sub.empty()) {
                    a.n_sub = uint32_t(std::min<size_t>(d.sub.size(), 4));
                    if (d.sub.size() > 4)
                        throw std::runtime_error(
                            ">4 metric sub-aggregations");
                    for (size_t si = 0; si < d.sub.size(); ++si) {
                        const FastFieldView* sf =
                            sv.fast_field(d.sub[si].field);
                        if (d.sub[si].kind == MetricAgg::PERCENTILES) {
                            // sketched by the second pass over the kept
                            // buckets (terms_perc_pass); here the slot stays
                            // an empty stats slot, like a missing column
                            if (sf && sf->type != FastFieldView::STR &&
                                !sf->multi) {
                                double mn, mx;
                                col_min_max(*sf, &mn, &mx);
                                if (mn < 0)
                                    throw std::runtime_error(
                                        "percentiles over negative values "
                                        "(r1 limit)");
                            }
                            a.sub_values_off[si] = 0;
                            a.sub_width[si] = 0;
                            continue;
                        }
                        if (sf && sf->type != FastFieldView::STR) {
                            a.sub_values_off[si] = sf->values.off;
                            a.sub_nulls_off[si] =
                                sf->nullable ? sf->nulls.off : 0;
                            a.sub_width[si] = 8;
                            a.sub_is_i64[si] =
                                sf->type == FastFieldView::U64   ? 0
                                : sf->type == FastFieldView::F64 ? 2
                                                                 : 1;
                        } else {
                            a.sub_values_off[si] = 0;
                            a.sub_width[si] = 0;
                        }
                    }
                }
            } else if (f && !f->multi) {
                // terms over a numeric fast column (tantivy term_agg keys by
                // the column value): device hash table sized so distinct
                // values can never fill it (<= num_docs). Bounded at 4M slots
                // — beyond that the per-doc worst-case probe cost is a
                // hazard, and no golden/benchmark path needs it.
                if (sv.num_docs > (1u << 21))
                    throw std::runtime_error(
                        "terms aggregation over a numeric fast field on a "
                        ">2M-doc split (r1 limit)");
                // numeric-keyed terms carry no sub-aggregations; a
                // percentiles sub would render as nulls, so it stays refused
                if (d.kind == AggDef::TERMS)
                    for (auto& s : d.sub)
                        if (s.kind == MetricAgg::PERCENTILES)
                            throw std::runtime_error(
                                "percentiles under terms over a numeric "
                                "column (r1 limit)");
                a.kind = AGGD_TERMS_NUM;
                uint64_t want = uint64_t(sv.num_docs) * 2;
                uint32_t slots = 1024;
                while (slots < want) slots <<= 1;
                a.n_buckets = slots * 2 + 2;
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = 8;
                a.value_is_i64 = f->type == FastFieldView::U64   ? 0
                                 : f->type == FastFieldView::F64 ? 2
                                                                 : 1;
            } else {
                a.n_buckets = 0;  // no such column: zero buckets
            }
        } else if (d.kind == AggDef::METRIC &&
                   d.metric.kind == MetricAgg::PERCENTILES) {
            a.kind = AGGD_PERC;
            if (f && f->type != FastFieldView::STR && !f->multi) {
                double mn, mx;
                col_min_max(*f, &mn, &mx);
                if (mn < 0)
                    throw std::runtime_error(
                        "percentiles over negative values (r1 limit)");
                int32_t k_lo = 0, k_hi = 0;
                if (mx >= PERC_MIN_VALUE) {
                    k_lo = perc_key_for(std::max(mn, PERC_MIN_VALUE));
                    k_hi = perc_key_for(mx);
                }
                a.p_k_lo = k_lo;
                a.p_n_keys = uint32_t(k_hi - k_lo + 1);
                a.n_buckets = a.p_n_keys + 1;  // + zero bucket word
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = 8;
                a.value_is_i64 = f->type == FastFieldView::U64   ? 0
                                 : f->type == FastFieldView::F64 ? 2
                                                                 : 1;
                perc_boundaries(k_lo, k_hi, ap.pbounds.back());
            }
        } else if (d.kind == AggDef::METRIC) {
            a.kind = AGGD_METRIC;
            if (f && f->type != FastFieldView::STR && !f->multi) {
                a.n_buckets = 1;  // one 40B stats slot at counts_out
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = 8;
                a.value_is_i64 = f->type == FastFieldView::U64   ? 0
                                 : f->type == FastFieldView::F64 ? 2
                                                                 : 1;
            }
        } else if (d.kind == AggDef::RANGE) {
            a.kind = AGGD_RANGE;
            if (f && f->type != FastFieldView::STR && !f->multi) {
                if (d.ranges.size() > AGG_MAX_RANGES)
                    throw std::runtime_error(">16 ranges in range aggregation");
                a.n_buckets = uint32_t(d.ranges.size());
                a.n_ranges = a.n_buckets;
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = 8;
                a.value_is_i64 = f->type == FastFieldView::U64   ? 0
                                 : f->type == FastFieldView::F64 ? 2
                                                                 : 1;
                for (size_t ri = 0; ri < d.ranges.size(); ++ri) {
                    if (d.ranges[ri].has_from) a.r_has_from |= 1u << ri;
                    if (d.ranges[ri].has_to) a.r_has_to |= 1u << ri;
                    a.r_from[ri] = d.ranges[ri].from;
                    a.r_to[ri] = d.ranges[ri].to;
                }
            }
        } else {
            a.kind = AGGD_HISTO;
            if (f && f->type != FastFieldView::STR) {
                a.interval = d.interval;
                a.offset = d.offset;
                a.values_off = f->values.off;
                a.nulls_off = f->nullable ? f->nulls.off : 0;
                a.value_width = 8;
                a.value_is_i64 = f->type == FastFieldView::U64   ? 0
                                 : f->type == FastFieldView::F64 ? 2
                                                                 : 1;
                double mn = double(f->min_value), mx = double(f->max_value);
                if (f->type == FastFieldView::U64) {
                    mn = double(uint64_t(f->min_value));
                    mx = double(uint64_t(f->max_value));
                } else if (f->type == FastFieldView::F64) {
                    mn = f->fmin;
                    mx = f->fmax;
                }
                int64_t b0 = int64_t(std::floor((mn - d.offset) / d.interval));
                int64_t b1 = int64_t(std::floor((mx - d.offset) / d.interval));
                a.base_index = b0;
                // exact integer fast path (kernels.hip histo_bucket): valid
                // when interval/offset are integral, the i64 load reads the
                // true value (u64 columns must fit i64), and |v-offset| stays
                // below 2^53 so the double division the oracle does can never
                // land within one rounding error of an integer other than at
                // exact multiples (error <= |v-off|*2^-53 < 1 < 1/interval
                // distance to the nearest non-multiple boundary).
                {
                    double iv = d.interval, of = d.offset;
                    bool integral = iv >= 1.0 && std::floor(iv) == iv &&
                                    std::floor(of) == of;
                    bool u64_ok = (f->type != FastFieldView::U64 ||
                                   uint64_t(f->max_value) < (1ull << 63)) &&
                                  f->type != FastFieldView::F64;
                    double span = std::max(std::fabs(mn - of), std::fabs(mx - of));
                    if (integral && u64_ok && span < 9.0e15 && iv < 9.0e15 &&
                        std::fabs(of) < 9.0e15 && std::fabs(mn) < 9.0e15 &&
                        std::fabs(mx) < 9.0e15) {
                        a.int_fast = 1;
                        a.i_interval = int64_t(iv);
                        a.i_offset = int64_t(of);
                        a.inv_interval = 1.0 / iv;
                    }
                }
                int64_t nb = b1 - b0 + 1;
                if (nb < 0 || nb > bucket_limit)
                    throw std::runtime_error(
                        "aggregation bucket limit exceeded (AggregationLimitsGuard)");
                a.n_buckets = uint32_t(nb);
                a.n_sub = uint32_t(std::min<size_t>(d.sub.size(), 4));
                if (d.sub.size() > 4)
                    throw std::runtime_error(">4 metric sub-aggregations");
                for (size_t si = 0; si < d.sub.size(); ++si) {
                    const FastFieldView* sf = sv.fast_field(d.sub[si].field);
                    if (sf && sf->type != FastFieldView::STR) {
                        a.sub_values_off[si] = sf->values.off;
                        a.sub_nulls_off[si] = sf->nullable ? sf->nulls.off : 0;
                        a.sub_width[si] = 8;
                        a.sub_is_i64[si] = sf->type == FastFieldView::U64   ? 0
                                           : sf->type == FastFieldView::F64 ? 2
                                                                            : 1;
                        if (d.sub[si].kind == MetricAgg::PERCENTILES) {
                            if (a.p_si != 0xFF)
                                throw std::runtime_error(
                                    ">1 percentiles sub-aggregation "
                                    "(r1 limit)");
                            double mn, mx;
                            col_min_max(*sf, &mn, &mx);
                            if (mn < 0)
                                throw std::runtime_error(
                                    "percentiles over negative values "
                                    "(r1 limit)");
                            int32_t k_lo = 0, k_hi = 0;
                            if (mx >= PERC_MIN_VALUE) {
                                k_lo = perc_key_for(
                                    std::max(mn, PERC_MIN_VALUE));
                                k_hi = perc_key_for(mx);
                            }
                            a.p_si = uint32_t(si);
                            a.p_k_lo = k_lo;
                            a.p_n_keys = uint32_t(k_hi - k_lo + 1);
                            if (uint64_t(a.n_buckets) * (a.p_n_keys + 1) >
                                (1ull << 25))
                                throw std::runtime_error(
                                    "percentiles sketch region too large "
                                    "(r1 limit)");
                            perc_boundaries(k_lo, k_hi, ap.pbounds.back());
                        }
                    } else {
                        a.sub_values_off[si] = 0;  // missing column: no values
                        a.sub_width[si] = 0;
                    }
                }
            } else {
                a.n_buckets = 0;
            }
        }
        // layout: counts u64[n_buckets] (METRIC: one stats slot) |
        // matched u64 | subs n_buckets*n_sub*STATS_SLOT_BYTES
        a.counts_out = off;
        off += a.kind == AGGD_METRIC ? STATS_SLOT_BYTES
                                     : uint64_t(a.n_buckets) * 8;
        a.matched_out = off;
        off += 8;
        a.sub_out = off;
        // AGGD_COMP uses n_sub for its sources and n_buckets for the hash
        // table words — no per-bucket stats region
        if (a.kind != AGGD_COMP)
            off += uint64_t(a.n_buckets) * a.n_sub * STATS_SLOT_BYTES;
        if (a.p_si != 0xFF) {
            a.p_out = off;
            off += uint64_t(a.n_buckets) * (a.p_n_keys + 1) * 8;
        }
        ap.devs.push_back(a);
    }
    // LDS slot assignment: the first histogram agg that fits gets the LDS
    // histogram array, the first terms agg that fits gets the LDS count
    // table; everything else accumulates with global atomics.
    bool slot0 = false, slot1 = false;
    for (AggDev& a : ap.devs) {
        a.lds_rep = 1;
        if (a.kind == AGGD_HISTO && !slot0 && a.n_buckets &&
            a.n_buckets <= AGG_LDS_BUCKETS) {
            a.lds_slot = 0;
            slot0 = true;
        } else if (a.kind == AGGD_TERMS && !slot1 && a.n_buckets &&
                   a.n_buckets <= AGG_LDS_BUCKETS) {
            a.lds_slot = 1;
            slot1 = true;
        }
        // two interleaved copies when they fit the LDS array: lane-parity
        // split halves same-bucket atomic serialization (Zipf ords)
        if (a.lds_slot <= 1 && a.n_buckets * 2 <= AGG_LDS_BUCKETS) a.lds_rep = 2;
    }
    ap.out_bytes = off - out_base;
    // init pattern: zeros except sub min slots = f64_sortable(+inf) pattern max
    ap.init.assign(ap.out_bytes, 0);
    for (size_t i = 0; i < ap.devs.size(); ++i) {
        const AggDev& a = ap.devs[i];
        uint64_t ones = ~0ull;
        if (a.kind == AGGD_METRIC && a.n_buckets) {
            uint64_t slot = a.counts_out - out_base;
            memcpy(&ap.init[slot + 16], &ones, 8);  // min: max sortable
        }
        if ((a.kind == AGGD_TERMS_NUM || a.kind == AGGD_COMP) && a.n_buckets) {
            // hash table: every key word starts at the empty sentinel ~0
            uint32_t slots = (a.n_buckets - 2) >> 1;
            for (uint32_t s2 = 0; s2 < slots; ++s2)
                memcpy(&ap.init[a.counts_out - out_base + uint64_t(s2) * 16],
                       &ones, 8);
        }
        // AGGD_COMP reuses n_sub for its sources and has NO stats sub region
        if (a.kind == AGGD_COMP) continue;
        for (uint64_t b = 0; b < a.n_buckets; ++b)
            for (uint32_t s = 0; s < a.n_sub; ++s) {
                if (s == a.p_si) continue;  // percentiles slot: stays zero
                uint64_t slot = a.sub_out - out_base +
                                (b * a.n_sub + s) * STATS_SLOT_BYTES;
                memcpy(&ap.init[slot + 16], &ones, 8);  // min slot: max sortable
                // max slot stays 0 (= most negative sortable)
            }
    }
    return ap;
}

// ------------------------------------------------------------ per-split search
struct SplitResult {
    uint64_t num_hits = 0;
    std::vector<pb::PartialHit> hits;
    IntermediateAggResults aggs;
    bool has_aggs = false;
    uint64_t micros = 0;
    std::string error;
    // required terms this SEGMENT proved absent; the caller populates the
    // absence cache only with terms absent from EVERY segment of the split
    std::vector<std::pair<std::string, std::string>> absent_required;
};

// sort specs, mirroring the oracle's (collector.rs:403-414 sort-key
// extraction; sorting.md None-last + GlobalDocId tie-break semantics)
struct SortSpec {
    enum Comp { DOC_ID, SCORE, FAST_FIELD } comp = DOC_ID;
    const FastFieldView* ff = nullptr;  // null: unknown field -> None values
    int order = 1;                      // 0 asc 1 desc
};

static pb::SortByValue sort_value_of(const SortSpec& s, uint32_t doc, float score) {
    pb::SortByValue v;
    switch (s.comp) {
        case SortSpec::DOC_ID:
            break;
        case SortSpec::SCORE:
            v.kind = pb::SortByValue::F64;
            v.f64 = double(score);
            break;
        case SortSpec::FAST_FIELD: {
            const FastFieldView* f = s.ff;
            if (!f || !f->present(doc)) break;
            if (f->type == FastFieldView::MIXED) {
                // echo the ORIGINAL typed value (true stays a bool, a u64
                // beyond 2^63 stays exact) — tags/raw sections
                uint64_t r = f->mixed_raw(doc);
                switch (f->mixed_tag(doc)) {
                    case 1:
                        v.kind = pb::SortByValue::I64;
                        v.i64 = int64_t(r);
                        break;
                    case 2:
                        v.kind = pb::SortByValue::F64;
                        memcpy(&v.f64, &r, 8);
                        break;
                    case 3:
                        v.kind = pb::SortByValue::BOOL;
                        v.boolean = r != 0;
                        break;
                    default:
                        v.kind = pb::SortByValue::U64;
                        v.u64 = r;
                }
            } else if (f->type == FastFieldView::U64) {
                v.kind = pb::SortByValue::U64;
                v.u64 = f->u64(doc);
            } else if (f->type == FastFieldView::DATETIME) {
                v.kind = pb::SortByValue::I64;
                v.i64 = f->i64(doc) * 1000000;  // ms -> ns (sorting.md default
                                                // output unix_timestamp_nanos)
            } else if (f->type == FastFieldView::STR) {
                v.kind = pb::SortByValue::U64;
                v.u64 = f->ord(doc);
            } else if (f->type == FastFieldView::F64) {
                v.kind = pb::SortByValue::F64;
                v.f64 = f->f64(doc);
            } else {
                v.kind = pb::SortByValue::I64;
                v.i64 = f->i64(doc);
            }
            break;
        }
    }
    return v;
}

// Evaluate a CACHE node's inner subtree into a device HitSet bitmap
// (tile-major u32 words) and memoize it per (split, fingerprint). The
// assembly mirrors the hot-path one minus scoring/aggs/top-K: the query
// shape becomes an unscored flattened boolean whose per-tile match bitset
// is stored via QueryDev::bitmap_out.
static uint8_t* resolve_hitset(qw_ctx* ctx, const DeviceSplit& ds,
                               const PlanNode& inner, const Schema& schema);

static void record_kernel_time(qw_ctx* ctx, const char* name, float ms);

// combine helper: dst op= src (op per k_bitmap_combine)
static void bitmap_combine(qw_ctx* ctx, uint8_t* dst, const uint8_t* src,
                           size_t bm_bytes, uint32_t op) {
    uint64_t words = bm_bytes / 4;
    uint32_t grid = uint32_t(std::min<uint64_t>(2048, (words + 255) / 256));
    hipLaunchKernelGGL(k_bitmap_combine, dim3(grid), dim3(256), 0, ctx->stream,
                       (uint32_t*)dst, (const uint32_t*)src, words, op);
}

// Recursive boolean evaluation over device bitmaps — the fallback for plan
// shapes the single-pass flattened kernel cannot express (nested booleans
// under must_not, presence/range in should position, …). Each sub-plan's
// bitmap is memoized in the (split, fingerprint) hitset cache, so repeated
// subtrees and repeated queries pay once. Unscored semantics only.
static uint8_t* bitmap_eval(qw_ctx* ctx, const DeviceSplit& ds,
                            const PlanNode& node, const Schema& schema) {
    const SplitView& sv = ds.view;
    try {
        return resolve_hitset(ctx, ds, node, schema);  // flattenable fast path
    } catch (const std::exception&) {
        if (node.kind != PlanNode::BOOL) throw;
    }
    if (node.minimum_should_match > 1)
        throw std::runtime_error(
            "minimum_should_match>1 over nested clauses (GPU r1)");
    uint32_t n_tiles = (sv.num_docs + TILE_DOCS - 1) / TILE_DOCS;
    size_t bm_bytes = size_t(n_tiles) * (TILE_DOCS / 32) * 4;
    std::string key = sv.split_id;
    key += '\0';
    key += std::to_string(sv.segment_ord);
    key += '\x1e';
    plan_fingerprint(node, key);
    uint8_t* bm = nullptr;
    qw_check_budget(ctx, bm_bytes);
    HIP_CHECK(hipMalloc(&bm, bm_bytes));
    bool has_req = !node.must.empty() || !node.filter.empty();
    bool first = true;
    for (auto* clauses : {&node.must, &node.filter})
        for (const PlanNode& c : *clauses) {
            uint8_t* cb = bitmap_eval(ctx, ds, c, schema);
            bitmap_combine(ctx, bm, cb, bm_bytes, first ? 3u : 0u);
            first = false;
        }
    int64_t msm = node.minimum_should_match;
    if (msm <= 0) msm = has_req ? 0 : 1;
    if (!node.should.empty() && msm > 0) {
        uint8_t* su = nullptr;
        qw_check_budget(ctx, bm_bytes);
        HIP_CHECK(hipMalloc(&su, bm_bytes));
        bool sfirst = true;
        for (const PlanNode& c : node.should) {
            uint8_t* cb = bitmap_eval(ctx, ds, c, schema);
            bitmap_combine(ctx, su, cb, bm_bytes, sfirst ? 3u : 1u);
            sfirst = false;
        }
        if (first) {
            bitmap_combine(ctx, bm, su, bm_bytes, 3u);
            first = false;
        } else bitmap_combine(ctx, bm, su, bm_bytes, 0u);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        (void)hipFree(su);
    }
    if (first) {
        // no positive clause: implicit match_all base (must_not-only)
        HIP_CHECK(hipMemsetAsync(bm, 0xFF, bm_bytes, ctx->stream));
        first = false;
    }
    for (const PlanNode& c : node.must_not) {
        uint8_t* cb = bitmap_eval(ctx, ds, c, schema);
        bitmap_combine(ctx, bm, cb, bm_bytes, 2u);
    }
    // mask the tail beyond num_docs (match_all memset covers padding bits)
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    {
        uint32_t ndocs = sv.num_docs;
        uint32_t full_words = ndocs / 32;
        size_t total_words = bm_bytes / 4;
        if (full_words < total_words) {
            std::vector<uint32_t> tail(total_words - full_words, 0);
            if (ndocs % 32)
                tail[0] = 0;  // recompute partial word below
            // read-modify host-side for the single partial word
            if (ndocs % 32) {
                uint32_t w = 0;
                HIP_CHECK(hipMemcpy(&w, bm + full_words * 4, 4,
                                    hipMemcpyDeviceToHost));
                w &= (1u << (ndocs % 32)) - 1u;
                tail[0] = w;
            }
            HIP_CHECK(hipMemcpy(bm + full_words * 4, tail.data(),
                                tail.size() * 4, hipMemcpyHostToDevice));
        }
    }
    ctx->hitsets.put(key, bm, bm_bytes);
    return bm;
}

// host image of a DFA in the layout k_dict_dfa_match reads (kernels.hip)
static std::vector<uint8_t> dfa_table_image(const rx::Dfa& dfa, DfaDev* d) {
    size_t next_bytes = dfa.next.size() * 2;
    size_t accept_off = dfa.accept_off();
    std::vector<uint8_t> img(dfa.table_bytes(), 0);
    memcpy(img.data(), dfa.class_of, 256);
    memcpy(img.data() + 256, dfa.next.data(), next_bytes);
    memcpy(img.data() + accept_off, dfa.accept.data(), dfa.accept.size() * 8);
    d->n_classes = dfa.n_classes;
    d->accept_off = uint32_t(accept_off);
    d->table_bytes = uint32_t(img.size());
    d->in_lds = img.size() <= 64 * 1024 ? 1u : 0u;
    return img;
}

// PlanNode::REGEX into the (allocated, not yet zeroed) bitmap `bm`
static void regex_hitset(qw_ctx* ctx, const DeviceSplit& ds, const PlanNode& n,
                         uint8_t* bm, size_t bm_bytes) {
    const SplitView& sv = ds.view;
    const TextFieldView* f = sv.text_field(n.field);
    HIP_CHECK(hipMemsetAsync(bm, 0, bm_bytes, ctx->stream));
    if (!f || !f->num_terms) {  // no such text field in this split: no hits
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return;
    }
    // memoised: planned once, evaluated once per split and segment
    std::shared_ptr<const rx::Dfa> dfa = rx::compile_cached(n.value);
    DfaDev dd{};
    std::vector<uint8_t> img = dfa_table_image(*dfa, &dd);

    // 1. DFA scan: scratch = table image | match words
    const uint32_t n_words = (f->num_terms + 63u) / 64u;
    const size_t match_off = img.size();  // multiple of 8
    qw_ensure_acct(ctx, ctx->d_scratch, match_off + size_t(n_words) * 8);
    HIP_CHECK(hipMemcpyAsync(ctx->d_scratch.p, img.data(), img.size(),
                             hipMemcpyHostToDevice, ctx->stream));
    dd.table = ctx->d_scratch.p;
    uint64_t* d_match = (uint64_t*)(ctx->d_scratch.p + match_off);
    {
        // 4 words per 256-thread block; the kernel strides over the rest, so
        // a staged table is loaded at most 1024 times
        uint32_t grid = std::min<uint32_t>(1024u, (n_words + 3u) / 4u);
        HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
        hipLaunchKernelGGL(k_dict_dfa_match, dim3(grid), dim3(256),
                           dd.in_lds ? dd.table_bytes : 0u, ctx->stream,
                           ds.d_image, f->term_offsets.off, f->term_bytes.off,
                           f->num_terms, dd, d_match);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
    }
    // 2. read back (num_terms / 8 bytes)
    std::vector<uint64_t> match(n_words);
    HIP_CHECK(hipMemcpyAsync(match.data(), d_match, size_t(n_words) * 8,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
        record_kernel_time(ctx, "k_dict_dfa_match", ms);
    }
    // 3. matched-term list + exclusive prefix of their block counts
    std::vector<uint32_t> up;  // terms[n] | blk_prefix[n + 1]
    std::vector<uint32_t> prefix(1, 0u);
    uint64_t total = 0;
    for (uint32_t w = 0; w < n_words; ++w)
        for (uint64_t bits = match[w]; bits; bits &= bits - 1) {
            uint32_t t = w * 64u + uint32_t(__builtin_ctzll(bits));
            if (t >= f->num_terms || !f->h_n_blocks[t]) continue;
            up.push_back(t);
            total += f->h_n_blocks[t];
            if (total > UINT32_MAX)
                throw std::runtime_error(
                    "regex matches more than 2^32 posting blocks");
            prefix.push_back(uint32_t(total));
        }
    if (up.empty()) return;  // nothing matched: the zeroed bitmap stands
    // 4. union
    const uint32_t n_matched = uint32_t(up.size());
    up.insert(up.end(), prefix.begin(), prefix.end());
    qw_ensure_acct(ctx, ctx->d_scratch, up.size() * 4);
    HIP_CHECK(hipMemcpyAsync(ctx->d_scratch.p, up.data(), up.size() * 4,
                             hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* d_terms = (const uint32_t*)ctx->d_scratch.p;
    uint32_t grid =
        uint32_t(std::min<uint64_t>(2048u, (total + 3u) / 4u));  // wave each
    HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
    hipLaunchKernelGGL(k_terms_union_bitmap, dim3(grid), dim3(256), 0,
                       ctx->stream, ds.d_image, f->skip_off.off, f->skip.off,
                       f->payload.off, d_terms, d_terms + n_matched, n_matched,
                       uint32_t(total), sv.num_docs, (uint32_t*)bm);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    record_kernel_time(ctx, "k_terms_union_bitmap", ms);
}

static uint8_t* resolve_hitset(qw_ctx* ctx, const DeviceSplit& ds,
                               const PlanNode& inner, const Schema& schema) {
    const SplitView& sv = ds.view;
    std::string key = sv.split_id;
    key += '\0';
    key += std::to_string(sv.segment_ord);
    key += '\x1e';
    plan_fingerprint(inner, key);
    if (uint8_t* bm = ctx->hitsets.get(key)) return bm;

    uint32_t n_tiles = (sv.num_docs + TILE_DOCS - 1) / TILE_DOCS;
    size_t bm_bytes = size_t(n_tiles) * (TILE_DOCS / 32) * 4;
    uint8_t* bm = nullptr;
    qw_check_budget(ctx, bm_bytes);
    HIP_CHECK(hipMalloc(&bm, bm_bytes));

    if (inner.kind == PlanNode::PHRASE) {
        // multi-token phrase (slop 0, full_text_query.rs phrase mode):
        // k_phrase_bitmap — one thread per posting of the driver token,
        // consecutive-position chain over the field's position streams
        const TextFieldView* f = sv.text_field(inner.field);
        bool none = !f;
        if (f && !f->has_positions) {
            (void)hipFree(bm);
            throw std::runtime_error(
                "phrase query needs record: position on field " + inner.field);
        }
        if (inner.phrase_toks.size() > PHRASE_MAX_TOKS) {
            (void)hipFree(bm);
            throw std::runtime_error("phrase longer than 8 tokens (r2 limit)");
        }
        // slop > 0 or a prefix last token: k_phrase_window_bitmap, one wave
        // per (driver posting, last-token alternative); DESIGN.md §7
        const bool window = inner.prefix_last || inner.slop > 0;
        const uint32_t slop = inner.prefix_last ? 0u : inner.slop;
        if (slop > PHRASE_MAX_SLOP) {
            (void)hipFree(bm);
            throw std::runtime_error(
                "phrase slop > 31 not supported (one wave holds the window)");
        }
        auto tok_dev = [&](int64_t tid) {
            PhraseTokDev td{};
            td.skip_off = f->skip.off + f->h_skip_off[tid];
            td.payload_off = f->payload.off;
            td.pos_start_off =
                f->pos_start.off + (f->h_skip_off[tid] / 16) * 4;
            td.positions_off = f->positions.off;
            td.n_blocks = f->h_n_blocks[tid];
            td.df = f->h_doc_freq[tid];
            return td;
        };
        PhraseDev p{};
        p.n_toks = uint32_t(inner.phrase_toks.size());
        p.num_docs = sv.num_docs;
        // the last token of a phrase prefix is no term: it is expanded below
        size_t n_exact = inner.phrase_toks.size() - (inner.prefix_last ? 1 : 0);
        for (size_t i = 0; i < n_exact && !none; ++i) {
            const std::string& tok = inner.phrase_toks[i];
            int64_t tid = f->find_term(tok.data(), tok.size());
            if (tid < 0) {
                none = true;  // absent token: phrase matches nothing
                break;
            }
            p.tok[i] = tok_dev(tid);
        }
        // last-token alternatives: the token itself, or the first
        // max_expansions dictionary terms (byte order) starting with it
        std::vector<PhraseTokDev> alts;
        if (window && !none) {
            if (inner.prefix_last) {
                const std::string& pre = inner.phrase_toks.back();
                auto term_at = [&](uint32_t t, size_t* len) {
                    *len = f->h_term_offsets[t + 1] - f->h_term_offsets[t];
                    return (const char*)f->h_term_bytes + f->h_term_offsets[t];
                };
                uint32_t lo = 0, hi = f->num_terms;  // first term >= prefix
                while (lo < hi) {
                    uint32_t mid = (lo + hi) / 2;
                    size_t sl;
                    const char* s = term_at(mid, &sl);
                    int c = memcmp(s, pre.data(), std::min(sl, pre.size()));
                    if (c < 0 || (c == 0 && sl < pre.size())) lo = mid + 1;
                    else hi = mid;
                }
                for (uint32_t t = lo;
                     t < f->num_terms && alts.size() < inner.max_expansions;
                     ++t) {
                    size_t sl;
                    const char* s = term_at(t, &sl);
                    if (sl < pre.size() || memcmp(s, pre.data(), pre.size()))
                        break;  // past the prefix's contiguous range
                    alts.push_back(tok_dev(t));
                }
            } else {
                alts.push_back(p.tok[p.n_toks - 1]);
            }
            if (alts.empty()) none = true;  // prefix without expansion
        }
        HIP_CHECK(hipMemsetAsync(bm, 0, bm_bytes, ctx->stream));
        const char* kname = nullptr;
        if (!window && !none && p.tok[0].df) {
            uint32_t grid =
                std::min<uint32_t>(2048, (p.tok[0].df + 255) / 256);
            kname = "k_phrase_bitmap";
            HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
            hipLaunchKernelGGL(k_phrase_bitmap, dim3(grid), dim3(256), 0,
                               ctx->stream, ds.d_image, p, (uint32_t*)bm);
            HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
        }
        if (window && !none && p.tok[0].df) {
            size_t alt_bytes = alts.size() * sizeof(PhraseTokDev);
            try {
                qw_ensure_acct(ctx, ctx->d_scratch, alt_bytes);
            } catch (...) {
                (void)hipFree(bm);
                throw;
            }
            HIP_CHECK(hipMemcpyAsync(ctx->d_scratch.p, alts.data(), alt_bytes,
                                     hipMemcpyHostToDevice, ctx->stream));
            // 256 CUs x 32 waves = 2048 resident 4-wave blocks: grid.y takes
            // up to 16 alternatives, grid.x what is left of the 2048; the
            // kernel strides over the rest of both
            uint32_t gy = uint32_t(std::min<size_t>(alts.size(), 16));
            uint32_t slots = p.tok[0].n_blocks * 128u;  // one wave each
            uint32_t gx = std::min<uint32_t>(2048u / gy, (slots + 3) / 4);
            kname = "k_phrase_window_bitmap";
            HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
            hipLaunchKernelGGL(k_phrase_window_bitmap, dim3(gx, gy), dim3(256),
                               0, ctx->stream, ds.d_image, p,
                               (const PhraseTokDev*)ctx->d_scratch.p,
                               uint32_t(alts.size()), slop, (uint32_t*)bm);
            HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        HIP_CHECK(hipGetLastError());
        if (kname) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
            record_kernel_time(ctx, kname, ms);
        }
        ctx->hitsets.put(key, bm, bm_bytes);
        return bm;
    }

    if (inner.kind == PlanNode::REGEX) {
        // regex (regex_query.rs -> AutomatonQuery): compile, DFA scan of the
        // field's dictionary on the device, read the per-term match bitmap
        // back, union the matched terms' postings — no cap on their number
        try {
            regex_hitset(ctx, ds, inner, bm, bm_bytes);
        } catch (...) {
            (void)hipFree(bm);
            throw;
        }
        ctx->hitsets.put(key, bm, bm_bytes);
        return bm;
    }

    FlatQuery fq;
    try {
        fq = flatten(sv, inner, false);
    } catch (...) {
        (void)hipFree(bm);
        throw;
    }
    for (const PlanNode* cn : fq.cache_nodes) {  // nested cache nodes
        PredDev p{};
        p.type = PRED_BITSET;
        p.abs_bitmap =
            (uint64_t)resolve_hitset(ctx, ds, cn->cache_inner.front(), schema);
        fq.preds.push_back(p);
    }
    if (fq.match_none) {
        HIP_CHECK(hipMemsetAsync(bm, 0, bm_bytes, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->hitsets.put(key, bm, bm_bytes);
        return bm;
    }

    // scratch: TermDev[] | PredDev[] | zero ktab | per-term block ranges
    std::vector<TermDev> terms(fq.terms.size());
    uint32_t n_must_not = 0;
    for (size_t i = 0; i < fq.terms.size(); ++i) {
        const FlatQuery::FTerm& t = fq.terms[i];
        TermDev& d = terms[i];
        d.role = t.role;
        d.grp = t.grp;
        d.n_blocks = t.f->h_n_blocks[t.tid];
        d.skip_off = t.f->skip.off + t.f->h_skip_off[t.tid];
        d.payload_off = t.f->payload.off;
        d.norms_off = 0;
        d.weight = 0.f;
        d.ktab_idx = 0;
        n_must_not += t.role == ROLE_MUST_NOT;
    }
    size_t off_terms = 0;
    size_t off_preds = off_terms + terms.size() * sizeof(TermDev);
    size_t off_ktabs = off_preds + fq.preds.size() * sizeof(PredDev);
    size_t scratch_bytes = off_ktabs + 256 * 4;
    for (size_t i = 0; i < fq.terms.size(); ++i) {
        const FlatQuery::FTerm& t = fq.terms[i];
        terms[i].ranges_addr =
            term_ranges_addr(ctx, ds, t.f, t.tid, n_tiles, sv.num_docs);
    }
    std::vector<uint8_t> scratch(scratch_bytes, 0);
    memcpy(scratch.data() + off_terms, terms.data(), terms.size() * sizeof(TermDev));
    memcpy(scratch.data() + off_preds, fq.preds.data(),
           fq.preds.size() * sizeof(PredDev));
    qw_ensure_acct(ctx, ctx->d_scratch, scratch_bytes);
    qw_ensure_acct(ctx, ctx->d_results, 64);
    HIP_CHECK(hipMemcpyAsync(ctx->d_scratch.p, scratch.data(), scratch_bytes,
                             hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_results.p, 0, 64, ctx->stream));

    uint32_t n_should = 0;
    for (auto& t : fq.terms) n_should += t.role == ROLE_SHOULD;
    QueryDev q{};
    q.split = ds.d_image;
    q.scratch = ctx->d_scratch.p;
    q.results = ctx->d_results.p;
    q.num_docs = sv.num_docs;
    q.n_tiles = n_tiles;
    q.n_terms = uint32_t(terms.size());
    q.n_must = fq.n_must_groups;
    q.n_must_not = n_must_not;
    q.n_preds = uint32_t(fq.preds.size());
    q.msm = fq.msm;
    q.match_all = fq.match_all ? 1 : 0;
    q.collect_hits = 1;
    q.terms_off = off_terms;
    q.preds_off = off_preds;
    q.ktabs_off = off_ktabs;
    q.tile_counts_off = 0;  // unused (do_count = 0)
    q.cand_count_off = 0;   // phase-B reservation counter only
    q.cand_off = 0;
    q.cand_cap = 0;  // no candidate writes, bitmap only
    q.bitmap_out = (uint64_t)bm;
    bool ns = n_should > 0;
    bool nb = fq.n_must_groups > 0 || n_must_not > 0;
    launch_leaf_tile(ns, nb, false, true, dim3(n_tiles), ctx->stream, q, 0u,
                     n_tiles, 0u);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->hitsets.put(key, bm, bm_bytes);
    return bm;
}

static uint32_t f32_sortable_h(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

static void record_kernel_time(qw_ctx* ctx, const char* name, float ms) {
    KernelTimer& t = ctx->timers[name];
    t.total_ms += ms;
    t.launches += 1;
}

// single terms in REQUIRED position (must/filter chains, unwrapping cache
// nodes) — the candidates the absence cache can short-circuit on; restates
// the reference's required-term extraction (quickwit-query required_terms
// feeding leaf.rs:769-778)
static void collect_required_terms(
    const PlanNode& n, std::vector<std::pair<std::string, std::string>>& out) {
    switch (n.kind) {
        case PlanNode::TERM:
            out.emplace_back(n.field, n.value);
            break;
        case PlanNode::PHRASE:
            // every phrase token is required (the phrase cannot match if
            // any token is absent), except a prefix last token: no term
            for (size_t i = 0; i + (n.prefix_last ? 1 : 0) < n.phrase_toks.size();
                 ++i)
                out.emplace_back(n.field, n.phrase_toks[i]);
            break;
        case PlanNode::BOOL:
            for (const PlanNode& c : n.must) collect_required_terms(c, out);
            for (const PlanNode& c : n.filter) collect_required_terms(c, out);
            break;
        case PlanNode::CACHE:
            if (!n.cache_inner.empty())
                collect_required_terms(n.cache_inner.front(), out);
            break;
        default:
            break;
    }
}

// ------------------------------------------------------------ leaf stages
// search_split_gpu (end of this section) is a short driver over the stages
// below. Each stage names its inputs and outputs; none keeps a reference
// into another stage's locals.

// QW_TIMING=1 stage log; logs are compared by label (profiles/README.md)
struct StageTimer {
    using Clock = std::chrono::steady_clock;
    Clock::time_point t0 = Clock::now(), tprev = t0;
    void mark(const char* what) {
        static const bool timing = getenv("QW_TIMING") != nullptr;
        if (!timing) return;
        auto now = Clock::now();
        fprintf(stderr, "[qw_timing] %-18s %8.1f us\n", what,
                std::chrono::duration_cast<std::chrono::nanoseconds>(now - tprev)
                        .count() /
                    1e3);
        tprev = now;
    }
    uint64_t micros() const {
        return uint64_t(std::chrono::duration_cast<std::chrono::microseconds>(
                            Clock::now() - t0)
                            .count());
    }
};

// request -> PlanNode: the query AST, the request's timestamp bounds as a
// RANGE filter, and the absence-cache short circuit
static PlanNode leaf_plan(qw_ctx* ctx, const SplitView& sv,
                          const pb::SearchRequest& req, const Schema& schema) {
    PlanNode plan = parse_query_ast(req.query_ast, schema);
    if ((req.start_timestamp || req.end_timestamp) && !schema.timestamp_field.empty()) {
        // leaf.rs:977 rewrite_request: [start,end) seconds over the ts column
        PlanNode ts;
        ts.kind = PlanNode::RANGE;
        ts.field = schema.timestamp_field;
        if (req.start_timestamp) {
            ts.lo.kind = Bound::INCLUDED;
            ts.lo.ival = *req.start_timestamp * 1000;
        }
        if (req.end_timestamp) {
            ts.hi.kind = Bound::EXCLUDED;
            ts.hi.ival = *req.end_timestamp * 1000;
        }
        PlanNode b;
        b.kind = PlanNode::BOOL;
        b.filter.push_back(std::move(ts));
        b.must.push_back(std::move(plan));
        plan = std::move(b);
    }

    // ---- negative/absence term cache probe (leaf.rs:761-827): a required
    // term proven absent by an earlier search short-circuits this split —
    // replace the plan with MATCH_NONE so the standard empty-response path
    // (shaped agg blob, stats) runs with no kernel and no dict lookups
    std::vector<std::pair<std::string, std::string>> reqs;
    collect_required_terms(plan, reqs);
    bool hit = false;
    for (auto& ft : reqs)
        if (ctx->absence.keys.count(
                AbsenceCache::key(sv.split_id, ft.first, ft.second))) {
            hit = true;
            break;
        }
    if (!reqs.empty()) (hit ? ctx->absence.hits : ctx->absence.misses)++;
    if (hit) {
        PlanNode none;
        none.kind = PlanNode::MATCH_NONE;
        plan = std::move(none);
    }
    return plan;
}

// sort orders of a request (0 asc, 1 desc); doc-id order defaults to desc
static void request_sort_orders(const pb::SearchRequest& req, int* order1,
                                int* order2) {
    *order1 = req.sort_fields.empty() ? 1 : req.sort_fields[0].sort_order;
    *order2 = req.sort_fields.size() > 1 ? req.sort_fields[1].sort_order : 1;
}

// how the request sorts, and its search_after cursor in the sort fields'
// u64 domains
struct SortPlan {
    std::vector<SortSpec> specs;
    int order1 = 1, order2 = 1;
    bool scoring = false;  // some sort field is _score
    // narrow (8B) candidate records embed the f32 _score key + doc tiebreak:
    // exact device-side selection. fast-field or two-field sorts use wide
    // (16B) records selected by primary key only; exact order over the
    // survivors is re-established on host (kernels.hip wide_sort_key).
    bool wide = false;
    // effective cursor: null when the request has none, or when it sorts
    // before every value (CursorKey::disabled)
    const pb::PartialHit* after = nullptr;
    CursorKey ck1, ck2;

    static SortFieldKind kind_of(const SortSpec& s) {
        if (s.comp == SortSpec::SCORE) return SortFieldKind::SCORE;
        if (s.comp != SortSpec::FAST_FIELD || !s.ff) return SortFieldKind::NONE;
        switch (s.ff->type) {
            case FastFieldView::U64: return SortFieldKind::U64;
            case FastFieldView::I64: return SortFieldKind::I64;
            case FastFieldView::DATETIME: return SortFieldKind::DATETIME;
            case FastFieldView::F64: return SortFieldKind::F64;
            case FastFieldView::MIXED: return SortFieldKind::MIXED;
            default: return SortFieldKind::STR;
        }
    }
    bool mixed(size_t i) const {
        return specs.size() > i && kind_of(specs[i]) == SortFieldKind::MIXED;
    }
    // ascending primary sort: candidate keys are flipped on the device.
    // make_sort_plan only ever sets comp to SCORE or FAST_FIELD, so a
    // `comp != DOC_ID` term would be implied by !specs.empty().
    bool sort_asc() const { return !specs.empty() && order1 == 0; }
};

static SortPlan make_sort_plan(const SplitView& sv, const pb::SearchRequest& req) {
    if (req.sort_fields.size() > 2)
        throw std::runtime_error("more than two sort fields (search.proto:269)");
    SortPlan sp;
    for (auto& sf : req.sort_fields) {
        SortSpec s;
        s.order = sf.sort_order;
        if (sf.field_name == "_score") s.comp = SortSpec::SCORE;
        else {
            s.comp = SortSpec::FAST_FIELD;
            s.ff = sv.fast_field(sf.field_name);
        }
        sp.scoring |= s.comp == SortSpec::SCORE;
        sp.specs.push_back(s);
    }
    request_sort_orders(req, &sp.order1, &sp.order2);
    sp.wide = (!sp.specs.empty() && sp.specs[0].comp == SortSpec::FAST_FIELD) ||
              sp.specs.size() > 1;
    // typed cursor conversion into the sort fields' u64 domains
    // (convert_to_u64_ff_val, collector.rs:214-340)
    if (req.search_after) {
        sp.after = &*req.search_after;
        if (!sp.specs.empty())
            sp.ck1 = convert_cursor_key(sp.after->sort_value,
                                        SortPlan::kind_of(sp.specs[0]), sp.order1);
        if (sp.specs.size() > 1)
            sp.ck2 = convert_cursor_key(sp.after->sort_value2,
                                        SortPlan::kind_of(sp.specs[1]), sp.order2);
        if (sp.ck1.disabled) sp.after = nullptr;  // cursor before all values
    }
    return sp;
}

// the combined gate bitmaps of one split search (AND of two or more node
// bitmaps; the node bitmaps themselves belong to the hitset cache). Counted
// in hbm_used while they live, freed when the search ends, by whatever exit.
struct GateBitmaps {
    qw_ctx* ctx;
    std::vector<std::pair<uint8_t*, size_t>> bms;
    explicit GateBitmaps(qw_ctx* c) : ctx(c) {}
    GateBitmaps(const GateBitmaps&) = delete;
    GateBitmaps& operator=(const GateBitmaps&) = delete;
    ~GateBitmaps() {
        for (auto& b : bms) {
            (void)hipFree(b.first);  // waits for the kernels reading it
            ctx->hbm_used -= b.second;
        }
    }
    uint8_t* alloc(size_t bytes) {
        qw_check_budget(ctx, bytes);
        uint8_t* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes));
        bms.emplace_back(p, bytes);
        ctx->hbm_used += bytes;
        return p;
    }
};

// Scored plan that does not flatten. The oracle's eval_bool
// scores a bool as boost * (sum of its matching must and should children),
// so a term leaf t adds W_t * tfnorm(t, d) iff d is in t's postings and every
// bool between t and the root matches d; W_t carries every boost on the path.
// The plan is match_all + PRED_BITSET(root match set) with every such leaf as
// an optional should term (msm 0) whose score is gated by the AND of those
// ancestors' match sets. Three facts shrink a gate:
//   - the root is the PRED_BITSET, which drops non-matching docs anyway;
//   - a bool reached over a must edge matches wherever its parent does;
//   - a pure OR of terms matches wherever one of its terms does.
// What is left is the bools reached over a should edge: none for most
// leaves, one memoized node bitmap for many, a combined temporary otherwise.
struct ScoredTreePlanner {
    qw_ctx* ctx;
    const DeviceSplit& ds;
    const Schema& schema;
    GateBitmaps& tmp;
    FlatQuery& fq;
    size_t bm_bytes;
    bool any_gate = false;

    void walk(const PlanNode& raw, float boost, const uint8_t* gate) {
        const PlanNode& n = uncache(raw);
        if (n.kind == PlanNode::TERM) {
            size_t before = fq.terms.size();
            add_term(fq, ds.view, n.field, n.value, ROLE_SHOULD, boost * n.boost,
                     true);
            if (fq.terms.size() == before) return;  // not in the dictionary
            if (fq.terms.back().weight <= 0.f)
                throw std::runtime_error("non-positive BM25 weight (boost<=0?)");
            fq.gates.push_back((uint64_t)gate);
            any_gate |= gate != nullptr;
            return;
        }
        if (n.kind != PlanNode::BOOL) return;  // matches, never scores
        boost *= n.boost;
        for (const PlanNode& c : n.must) walk(c, boost, gate);
        for (const PlanNode& c_raw : n.should) {
            const PlanNode& c = uncache(c_raw);
            const uint8_t* g = gate;
            if (c.kind == PlanNode::BOOL && !is_pure_should_terms(c)) {
                const uint8_t* node_bm = bitmap_eval(ctx, ds, c, schema);
                if (!gate) {
                    g = node_bm;
                } else {
                    uint8_t* both = tmp.alloc(bm_bytes);
                    bitmap_combine(ctx, both, node_bm, bm_bytes, 3u);
                    bitmap_combine(ctx, both, gate, bm_bytes, 0u);
                    g = both;
                }
            }
            walk(c, boost, g);
        }
    }
};

static FlatQuery scored_tree_plan(qw_ctx* ctx, const DeviceSplit& ds,
                                  const PlanNode& plan, const Schema& schema,
                                  GateBitmaps& tmp) {
    FlatQuery fq;
    fq.scoring = true;
    fq.match_all = true;
    fq.msm = 0;  // the shoulds only add score; the bitmap decides the match
    PredDev p{};
    p.type = PRED_BITSET;
    p.abs_bitmap = (uint64_t)bitmap_eval(ctx, ds, plan, schema);
    fq.preds.push_back(p);
    uint32_t n_tiles = (ds.view.num_docs + TILE_DOCS - 1) / TILE_DOCS;
    ScoredTreePlanner pl{ctx, ds, schema, tmp, fq,
                         size_t(n_tiles) * (TILE_DOCS / 32) * 4};
    pl.walk(plan, 1.f, nullptr);
    if (!pl.any_gate) fq.gates.clear();
    return fq;
}

// plan -> FlatQuery, with every bitmap-backed predicate resolved
static FlatQuery flatten_or_bitmap(qw_ctx* ctx, const DeviceSplit& ds,
                                   const PlanNode& plan, const Schema& schema,
                                   bool scoring, GateBitmaps& gate_tmp) {
    FlatQuery fq;
    try {
        fq = flatten(ds.view, plan, scoring);
    } catch (const NotFlattenable& e) {
        if (scoring) {
            if (e.why != NotFlattenable::TREE) throw;
            return scored_tree_plan(ctx, ds, plan, schema, gate_tmp);
        }
        // unscored plan the single-pass kernel cannot express: evaluate the
        // whole boolean recursively into a device bitmap and search
        // match_all + PRED_BITSET (results identical; scores don't exist)
        uint8_t* bmp = bitmap_eval(ctx, ds, plan, schema);
        fq = FlatQuery{};
        fq.scoring = false;
        fq.match_all = true;
        PredDev p{};
        p.type = PRED_BITSET;
        p.abs_bitmap = (uint64_t)bmp;
        fq.preds.push_back(p);
    }
    // CACHE nodes in filter position -> device HitSet bitmaps (PRED_BITSET)
    for (const PlanNode* cn : fq.cache_nodes) {
        PredDev p{};
        p.type = PRED_BITSET;
        p.abs_bitmap =
            (uint64_t)bitmap_eval(ctx, ds, cn->cache_inner.front(), schema);
        fq.preds.push_back(p);
    }
    return fq;
}

// AggResult::kind of an aggregation (qagg_format.h)
static uint8_t agg_result_kind(const AggDef& d) {
    switch (d.kind) {
        case AggDef::TERMS:
        case AggDef::CARDINALITY:
        case AggDef::COMPOSITE: return 3;
        case AggDef::RANGE: return 4;
        case AggDef::METRIC:
            return d.metric.kind == MetricAgg::PERCENTILES ? 6 : 5;
        case AggDef::HISTOGRAM: return 2;
        case AggDef::DATE_HISTOGRAM: return 1;
    }
    return 1;
}

// empty-but-shaped blob, like the oracle over an empty match set. Unlike
// decode_aggs it tags sub_kinds for every aggregation kind: plan_aggs never
// ran here, so the combinations it rejects are still encoded as requested.
static void empty_agg_shapes(const std::string& agg_json,
                             IntermediateAggResults& out) {
    for (const AggDef& d : parse_agg_request(agg_json)) {
        AggResult r;
        r.name = d.name;
        r.kind = agg_result_kind(d);
        if (d.kind == AggDef::COMPOSITE) r.key_kind = 9;
        for (auto& s : d.sub) {
            r.sub_names.push_back(s.name);
            r.sub_kinds.push_back(s.kind == MetricAgg::PERCENTILES ? 1 : 0);
        }
        out.aggs.push_back(std::move(r));
    }
}

// device term descriptors + the BM25 K tables they index
struct TermTables {
    std::vector<TermDev> terms;
    std::vector<float> ktabs;  // 256 f32 per fq.ktab_fields entry, >= 1 table
    uint32_t n_must = 0, n_must_not = 0;
};

static TermTables build_term_tables(const SplitView& sv, FlatQuery& fq) {
    TermTables tt;
    tt.terms.resize(fq.terms.size());
    for (size_t i = 0; i < fq.terms.size(); ++i) {
        const FlatQuery::FTerm& t = fq.terms[i];
        TermDev& d = tt.terms[i];
        d.role = t.role;
        d.n_blocks = t.f->h_n_blocks[t.tid];
        d.skip_off = t.f->skip.off + t.f->h_skip_off[t.tid];
        d.payload_off = t.f->payload.off;
        d.norms_off = t.f->has_norms ? t.f->fieldnorms.off : 0;
        d.weight = t.weight;
        d.grp = t.grp;
        // K tables per field actually referenced by scored terms
        d.ktab_idx = fq.scoring ? fq.ktab_for(t.f) : 0;
        tt.n_must += t.role == ROLE_MUST;
        tt.n_must_not += t.role == ROLE_MUST_NOT;
    }
    tt.ktabs.resize(std::max<size_t>(1, fq.ktab_fields.size()) * 256, 0.f);
    for (size_t k = 0; k < fq.ktab_fields.size(); ++k) {
        const TextFieldView* f = fq.ktab_fields[k];
        double avgdl = f->total_tokens > 0 && sv.num_docs > 0
                           ? double(f->total_tokens) / double(sv.num_docs)
                           : 0.0;
        const double K1 = 1.2, B = 0.75;
        for (int i = 0; i < 256; ++i) {
            double fn = double(FIELDNORM_TABLE.v[i]);
            tt.ktabs[k * 256 + i] =
                float(K1 * (1.0 - B + B * fn / (avgdl > 0 ? avgdl : 1.0)));
        }
    }
    return tt;
}

// byte offsets of one query's two device regions
struct ScratchLayout {
    // query scratch (one H2D): TermDev[] | PredDev[] | AggDev[] | K tables |
    // percentiles boundary tables | term gates (scored tree plans)
    size_t off_terms = 0, off_preds = 0, off_aggs = 0, off_ktabs = 0;
    size_t off_gates = 0;  // 0 = no gated term
    size_t scratch_bytes = 0;
    // results: tile counts | 64 B cand_count header (gpu_types.h) | selection
    // histogram | aggregation output | candidate records
    size_t r_tile_counts = 0, r_cand_count = 0, r_hist = 0, r_agg = 0, r_cand = 0;
    size_t results_bytes = 0;
    size_t cand_cap = 0;  // candidate records (0 = no collection)
    size_t cand_rec = 8;  // bytes per record
};

// the results offsets up to r_agg depend on the tile count alone; plan_aggs
// needs r_agg as its output base before the rest can be laid out
static ScratchLayout layout_results_head(uint32_t n_tiles) {
    ScratchLayout L;
    L.r_tile_counts = 0;
    L.r_cand_count = L.r_tile_counts + size_t(n_tiles) * 4;
    L.r_cand_count = (L.r_cand_count + 63) & ~size_t(63);
    L.r_hist = L.r_cand_count + 64;
    L.r_agg = L.r_hist + TOPK_BINS * 4;
    L.r_agg = (L.r_agg + 63) & ~size_t(63);
    return L;
}

// completes the layout; also places each percentiles boundary table
// (gamma^k doubles the kernel searches) and records it in ap.devs
static void layout_finish(ScratchLayout& L, const TermTables& tt,
                          const FlatQuery& fq, AggPlan& ap, size_t cand_cap,
                          bool wide) {
    L.r_cand = L.r_agg + ((ap.out_bytes + 63) & ~size_t(63));
    L.cand_cap = cand_cap;
    L.cand_rec = wide ? 16 : 8;
    L.results_bytes = L.r_cand + L.cand_cap * L.cand_rec;

    L.off_terms = 0;
    L.off_preds = L.off_terms + tt.terms.size() * sizeof(TermDev);
    L.off_aggs = L.off_preds + fq.preds.size() * sizeof(PredDev);
    L.off_ktabs = L.off_aggs + ap.devs.size() * sizeof(AggDev);
    L.scratch_bytes = L.off_ktabs + tt.ktabs.size() * 4;
    L.scratch_bytes = (L.scratch_bytes + 7) & ~size_t(7);
    for (size_t i = 0; i < ap.devs.size(); ++i)
        if (!ap.pbounds[i].empty()) {
            ap.devs[i].p_bound_off = L.scratch_bytes;
            L.scratch_bytes += ap.pbounds[i].size() * 8;
        }
    if (!fq.gates.empty()) {
        L.off_gates = L.scratch_bytes;  // 8-aligned, past the K tables: never 0
        L.scratch_bytes += fq.gates.size() * 8;
    }
}

// dense positive base => eager predicate evaluation (kernels.hip):
// estimate the pre-predicate match density from the term dfs
static void eager_pred_flags(const SplitView& sv, FlatQuery& fq) {
    double density = 1.0;
    if (!fq.match_all && !fq.terms.empty()) {
        double n = double(std::max<uint32_t>(sv.num_docs, 1));
        double mind = 1.0, sum = 0.0;
        bool has_must = false;
        for (const FlatQuery::FTerm& t : fq.terms) {
            double dfr = double(t.f->h_doc_freq[t.tid]) / n;
            if (t.role == ROLE_MUST) {
                mind = std::min(mind, dfr);
                has_must = true;
            } else if (t.role == ROLE_SHOULD) sum += dfr;
        }
        density = has_must ? mind
                  : fq.msm > 0 ? std::min(1.0, sum)
                               : 1.0;
    }
    if (density >= 0.15)
        for (PredDev& pr : fq.preds)
            if (pr.type == PRED_RANGE_U64 || pr.type == PRED_RANGE_I64 ||
                pr.type == PRED_RANGE_F64)
                pr.flags |= PRED_EAGER;
}

static void assemble_scratch(uint8_t* scratch, const ScratchLayout& L,
                             const TermTables& tt, const FlatQuery& fq,
                             const AggPlan& ap) {
    memcpy(scratch + L.off_terms, tt.terms.data(),
           tt.terms.size() * sizeof(TermDev));
    memcpy(scratch + L.off_preds, fq.preds.data(),
           fq.preds.size() * sizeof(PredDev));
    memcpy(scratch + L.off_aggs, ap.devs.data(), ap.devs.size() * sizeof(AggDev));
    memcpy(scratch + L.off_ktabs, tt.ktabs.data(), tt.ktabs.size() * 4);
    for (size_t i = 0; i < ap.devs.size(); ++i)
        if (!ap.pbounds[i].empty())
            memcpy(scratch + ap.devs[i].p_bound_off, ap.pbounds[i].data(),
                   ap.pbounds[i].size() * 8);
    if (L.off_gates)
        memcpy(scratch + L.off_gates, fq.gates.data(), fq.gates.size() * 8);
}

// everything launch_leaf_tile needs for one query
struct TileLaunch {
    QueryDev q{};
    // query-shape flags select the template instantiation whose dynamic
    // LDS holds exactly the sections this shape touches (kernels.hip)
    bool ns = false, nb = false, na = false;
    uint32_t grid = 0;
    const char* kname = "";  // kernel timer name
};

// reads ctx->d_scratch / ctx->d_results: both must be sized already
static TileLaunch fill_query_dev(qw_ctx* ctx, const DeviceSplit& ds,
                                 const FlatQuery& fq, const SortPlan& sp,
                                 const TermTables& tt, const AggPlan& ap,
                                 const ScratchLayout& L, bool collect,
                                 bool do_aggs, uint64_t leaf_max_hits,
                                 uint32_t n_tiles) {
    TileLaunch tl;
    QueryDev& q = tl.q;
    q.split = ds.d_image;
    q.scratch = ctx->d_scratch.p;
    q.results = ctx->d_results.p;
    q.num_docs = ds.view.num_docs;
    q.n_tiles = n_tiles;
    q.n_terms = uint32_t(tt.terms.size());
    q.n_must = fq.n_must_groups;  // group count (TermDev::grp)
    q.n_must_not = tt.n_must_not;
    q.n_preds = uint32_t(fq.preds.size());
    q.n_aggs = uint32_t(ap.devs.size());
    q.msm = fq.msm;
    q.scoring = fq.scoring ? 1 : 0;
    q.match_all = fq.match_all ? 1 : 0;
    q.collect_hits = collect ? 1 : 0;
    q.sort_asc = sp.sort_asc() ? 1 : 0;
    q.wide_cand = sp.wide ? 1 : 0;
    if (sp.wide) {
        const SortSpec& s0 = sp.specs[0];
        if (s0.comp == SortSpec::SCORE) {
            q.sort_src = 1;
        } else if (s0.ff) {
            const FastFieldView* f = s0.ff;
            if (f->multi)
                throw std::runtime_error(
                    "sort by a multi-valued fast field not supported");
            q.sort_values_off = f->values.off;
            q.sort_nulls_off = f->nullable ? f->nulls.off : 0;
            if (f->type == FastFieldView::STR) {
                q.sort_src = 2;
                q.sort_width = uint32_t(f->ord_width);
            } else {
                // MIXED columns store f64-monotonic u64 keys: ascending
                // u64 order IS the numeric order -> device treats them
                // like a u64 column
                q.sort_src = f->type == FastFieldView::U64    ? 2
                             : f->type == FastFieldView::MIXED ? 2
                             : f->type == FastFieldView::F64  ? 4
                                                              : 3;
                q.sort_width = 8;
            }
        } else {
            q.sort_src = 0;  // unknown field: every key is None
        }
    }
    q.terms_off = L.off_terms;
    q.preds_off = L.off_preds;
    q.aggs_off = L.off_aggs;
    q.ktabs_off = L.off_ktabs;
    // LDS staging of fieldnorms + K tables for the scoring decode path
    // (kernels.hip): enabled when every scored term's norms live in ONE
    // section (single-field queries — the flagship shape) and the K
    // tables fit the LDS budget. QW_NO_LDS_NORMS / QW_NO_LDS_KTAB are
    // perf-experiment kill switches.
    if (fq.scoring) {
        // measured on MI355X at the 100M flagship: norms staging LOSES
        // (the +8KB LDS drops occupancy 4->3 WGs/CU while the norm
        // gathers already hit L2 — union covers ~25% of docs, ~16 hits
        // per cacheline); ktab staging is noise. Both stay available as
        // opt-in experiment switches (gpurun_out/r02_exp_variants.log).
        static const bool want_norms = getenv("QW_LDS_NORMS") != nullptr;
        static const bool want_ktab = getenv("QW_LDS_KTAB") != nullptr;
        uint64_t common = 0;
        bool uniform = true;
        for (const TermDev& t : tt.terms)
            if (t.norms_off) {
                if (!common) common = t.norms_off;
                else if (common != t.norms_off) uniform = false;
            }
        q.norms_stage_off = (want_norms && uniform) ? common : 0;
        q.n_ktabs = (want_ktab && fq.ktab_fields.size() <= KTAB_LDS_MAX)
                        ? uint32_t(fq.ktab_fields.size())
                        : 0;
    }
    q.tile_counts_off = L.r_tile_counts;
    q.cand_count_off = L.r_cand_count;
    q.cand_off = L.r_cand;
    q.cand_cap = L.cand_cap;
    q.hist_off = L.r_hist;
    // prune candidates in the tile kernel: narrow records, small K, no
    // cursor (the cursor band is cut out of ALL candidates afterwards),
    // and a real candidate array
    if (collect && !sp.wide && !sp.after && L.cand_cap > 0 && leaf_max_hits >= 1 &&
        leaf_max_hits <= TOPK_PRUNE_MAX_K && ctx->topk_prune)
        q.prune_k = uint32_t(leaf_max_hits);

    // gated should terms: pruning stays on, its bound comes from the final
    // keys of matched docs, whatever summed into their scores
    q.gates_off = uint32_t(L.off_gates);
    tl.kname = L.off_gates         ? "union_bm25_gated"
               : !fq.terms.empty() ? "union_bm25"
               : do_aggs           ? "column_agg"
                                   : "range_filter";
    uint32_t n_should = uint32_t(tt.terms.size()) - tt.n_must - tt.n_must_not;
    tl.ns = n_should > 0 || (fq.scoring && !tt.terms.empty());
    tl.nb = tt.n_must > 0 || tt.n_must_not > 0;
    tl.na = do_aggs && !ap.devs.empty();
    // agg workloads: capped grid so the once-per-workgroup LDS flush
    // stays cheap (each WG owns several tiles). For PURE column scans
    // (no posting decode) the grid also scales DOWN with the split
    // size — the flush costs grid x buckets global atomics regardless
    // of docs, which dominated small splits (256 WGs x 4 waves still
    // fill the chip's 1024 resident-wave slots). Decode-carrying
    // kernels keep the wide grid: fewer WGs serialize the per-tile
    // decode loops and cost more than the flush saves (measured,
    // config5 ablation).
    tl.grid = n_tiles;
    if (tl.na)
        tl.grid = fq.terms.empty()
                      ? std::min<uint32_t>(
                            {n_tiles, 2048u, std::max<uint32_t>(256u, n_tiles / 8)})
                      : std::min<uint32_t>(n_tiles, 2048u);
    // straight-line agg path (kernels.hip): histo[0] int_fast LDS
    // non-nullable no-subs (+ optional terms[1] LDS non-nullable)
    if (tl.na && !ap.devs.empty() && ap.devs[0].kind == AGGD_HISTO &&
        ap.devs[0].lds_slot == 0 && ap.devs[0].int_fast &&
        ap.devs[0].n_sub == 0 && ap.devs[0].nulls_off == 0 &&
        ap.devs.size() <= 2 &&
        (ap.devs.size() < 2 ||
         (ap.devs[1].kind == AGGD_TERMS && ap.devs[1].lds_slot == 1 &&
          ap.devs[1].nulls_off == 0 && ap.devs[1].offsets_off == 0 &&
          ap.devs[1].n_buckets > 0)))
        q.agg_fast = 1;
    // terms-only straight-line path (config5's shape): one LDS terms
    // agg, non-nullable single-valued ord column, no subs
    if (tl.na && ap.devs.size() == 1 && ap.devs[0].kind == AGGD_TERMS &&
        ap.devs[0].lds_slot == 1 && ap.devs[0].n_sub == 0 &&
        ap.devs[0].nulls_off == 0 && ap.devs[0].offsets_off == 0 &&
        ap.devs[0].n_buckets > 0)
        q.agg_fast = 1;
    static const bool agg_nt = getenv("QW_AGG_NT") != nullptr;
    q.agg_nt = agg_nt ? 1 : 0;
    static const bool nt_decode = getenv("QW_NT_DECODE") != nullptr;
    q.nt_decode = nt_decode ? 1 : 0;
    return tl;
}

// the wide/narrow choice of each selection kernel, once
static void launch_cand_hist(bool wide, uint32_t grid, hipStream_t stream,
                             const uint64_t* cand, const uint32_t* n_ptr,
                             uint64_t prefix, uint32_t prefix_bits,
                             uint32_t* hist) {
    if (wide)
        hipLaunchKernelGGL(k_cand_hist_w, dim3(grid), dim3(256), 0, stream, cand,
                           n_ptr, prefix, prefix_bits, hist);
    else
        hipLaunchKernelGGL(k_cand_hist, dim3(grid), dim3(256), 0, stream, cand,
                           n_ptr, prefix, prefix_bits, hist);
}
static void launch_cand_compact(bool wide, uint32_t grid, hipStream_t stream,
                                const uint64_t* cand, uint32_t n,
                                uint64_t floor_key, uint64_t ceil_key,
                                uint64_t* out, uint32_t* out_count, uint32_t cap) {
    if (wide)
        hipLaunchKernelGGL(k_cand_compact_w, dim3(grid), dim3(256), 0, stream,
                           cand, n, floor_key, ceil_key, out, out_count, cap);
    else
        hipLaunchKernelGGL(k_cand_compact, dim3(grid), dim3(256), 0, stream, cand,
                           n, floor_key, ceil_key, out, out_count, cap);
}
static void launch_cand_pick_compact(bool wide, uint32_t grid, hipStream_t stream,
                                     const uint64_t* cand, uint32_t cand_cap,
                                     uint32_t* hdr, const uint32_t* hist,
                                     uint32_t kwant, uint64_t* out, uint32_t cap) {
    if (wide)
        hipLaunchKernelGGL(k_cand_pick_compact_w, dim3(grid),
                           dim3(TOPK_PICK_THREADS), 0, stream, cand, cand_cap, hdr,
                           hist, kwant, out, cap);
    else
        hipLaunchKernelGGL(k_cand_pick_compact, dim3(grid),
                           dim3(TOPK_PICK_THREADS), 0, stream, cand, cand_cap, hdr,
                           hist, kwant, out, cap);
}

// inclusive upper bound, in device-key space, of the search_after cursor's
// primary-value band (ties and the (v2, split, seg, doc) chain are settled
// by the exact host filter at hit building)
static uint64_t cursor_ceil_key(const SortPlan& sp, bool fq_scoring) {
    const SortKey& k1 = sp.ck1.key;  // converted to the field domain
    if (sp.wide) {
        if (!k1.has) return 0;  // cursor in the None region
        uint64_t S = k1.key;
        if (sp.specs[0].comp == SortSpec::SCORE) {
            uint32_t kh = f32_sortable_h(float(u64_to_f64(S)));
            S = (uint64_t(kh) << 32) | 0xFFFFFFFFull;
        } else if (sp.specs[0].ff &&
                   sp.specs[0].ff->type == FastFieldView::DATETIME) {
            int64_t ns = u64_to_i64(S);  // cursor carries ns
            int64_t ms = ns / 1000000 - ((ns % 1000000) < 0 ? 1 : 0);
            S = i64_to_u64(ms);
        }
        // I64/F64: same u64 map as the device key; U64/STR ord: identity
        return sp.order1 == 0 ? ~S : S;
    }
    uint32_t kh = 0;
    if (fq_scoring && k1.has) kh = f32_sortable_h(float(u64_to_f64(k1.key)));
    if (sp.sort_asc()) kh = ~kh;
    return (uint64_t(kh) << 32) | 0xFFFFFFFFull;
}

// top-K selection over the candidate records (device histogram refinement
// + host exact sort of the survivors; top_k_collector.rs semantics). Owns
// the state the growing-K retry of build_hits steers.
struct TopkSelector {
    qw_ctx* ctx;
    bool wide, after;        // after: an effective search_after cursor
    uint32_t rw;             // u64 words per candidate record
    uint64_t leaf_max_hits;
    uint64_t* d_cand = nullptr;  // records selected from: all candidates,
                                 // or the cursor band once compacted
    uint32_t* d_n = nullptr;     // device-side count of those records
    uint32_t* d_hist = nullptr;
    // cand_count header words (gpu_types.h)
    uint32_t *d_candidates = nullptr, *d_survivors = nullptr, *d_band = nullptr;
    // prefetched selection pass-0 histogram, in pinned staging (async D2H
    // to pageable memory degrades to a blocking staged copy)
    uint32_t* hist0;
    bool hist0_valid = false;
    uint64_t band_n = 0;  // records in d_cand
    uint64_t kwant = 0;   // K of the last select()
    std::vector<uint64_t> top_keys;  // survivors (narrow: sorted best-first)
    // one-sync selection: the device picked the floor key and compacted
    // behind pass 0, and the first TOPK_INLINE_SURVIVORS survivor records
    // came down with the main synchronize
    uint32_t* d_hdr = nullptr;       // cand_count header as u32 words
    uint32_t cand_cap = 0;           // candidate array capacity, records
    uint32_t surv_cap = 0;           // ctx->d_survivors capacity, records
    bool onesync = false;            // this call enqueued the one-sync batch
    uint32_t picked_survivors = 0;   // valid while `onesync`

    TopkSelector(qw_ctx* c, bool wide_, bool after_, uint64_t leaf_max_hits_)
        : ctx(c), wide(wide_), after(after_), rw(wide_ ? 2 : 1),
          leaf_max_hits(leaf_max_hits_) {
        ctx->h_surv.ensure(TOPK_BINS * 4);
        hist0 = (uint32_t*)ctx->h_surv.p;
    }

    // ctx->d_results must be sized for L already
    void attach(const ScratchLayout& L) {
        uint8_t* hdr = ctx->d_results.p + L.r_cand_count;
        d_cand = (uint64_t*)(ctx->d_results.p + L.r_cand);
        d_hist = (uint32_t*)(ctx->d_results.p + L.r_hist);
        d_candidates = cand_hdr_candidates(hdr);
        d_survivors = cand_hdr_survivors(hdr);
        d_band = cand_hdr_cursor_band(hdr);
        d_n = d_candidates;
        d_hdr = (uint32_t*)hdr;
        cand_cap = uint32_t(L.cand_cap);
    }

    // enqueue histogram pass 0 behind the main kernel (count read
    // device-side) so its result arrives with the same synchronize
    // (kept when pruning: the 100M flagship still emits ~130k records,
    // above the 16384 no-refinement threshold, and a pass over that few
    // costs far less than the extra round trip select() would need).
    // `prezeroed`: the histogram still holds the zeros of the results reset
    // (enqueue_uploads), nothing has written it since.
    void enqueue_pass0(uint32_t num_docs, bool prezeroed = false) {
        if (!prezeroed)
            HIP_CHECK(hipMemsetAsync(d_hist, 0, TOPK_BINS * 4, ctx->stream));
        // candidate count is device-side only at this point: size the
        // grid for the worst case (every doc a candidate)
        uint32_t hgrid = std::min<uint32_t>(512, (num_docs + 4095) / 4096);
        launch_cand_hist(wide, hgrid, ctx->stream, d_cand, d_candidates, 0ull, 0u,
                         d_hist);
    }

    // the two-sync flow's download of pass 0, into its own staging
    void download_pass0() {
        HIP_CHECK(hipMemcpyAsync(hist0, d_hist, TOPK_BINS * 4,
                                 hipMemcpyDeviceToHost, ctx->stream));
        hist0_valid = true;
    }

    // one-sync selection serves collecting calls without a search_after
    // cursor (the cursor band is cut out of all candidates first)
    bool onesync_wanted(bool collect) const {
        return collect && !after && ctx->topk_onesync;
    }

    // One-sync selection, step 1, before anything is enqueued (growing a
    // device buffer synchronizes): room for every survivor list the device
    // pick can leave. It compacts at most T = max(4 K, TOPK_REFINE_MIN)
    // records, K <= min(leaf_max_hits, num_docs), never more than there are
    // candidates (<= num_docs), and the inline download reads
    // TOPK_INLINE_SURVIVORS records whatever the count.
    void reserve_onesync(uint32_t num_docs) {
        uint64_t k = std::min<uint64_t>(leaf_max_hits, num_docs);
        uint64_t t = std::min<uint64_t>(std::max<uint64_t>(4 * k, TOPK_REFINE_MIN),
                                        num_docs);
        surv_cap = uint32_t(std::max<uint64_t>(t, TOPK_INLINE_SURVIVORS));
        qw_ensure_acct(ctx, ctx->d_survivors, size_t(surv_cap) * 8 * rw + 16);
        ctx->h_topk.ensure(size_t(TOPK_INLINE_SURVIVORS) * 8 * rw);
    }

    // step 2, behind the tile kernel: pass 0, then the pick and the
    // compaction in one launch (k_cand_pick_compact), then the inline
    // survivors. The histogram and the survivor counter still hold the zeros
    // of the results reset. `few`: the tile kernel pruned, so the candidates
    // are few and a small grid keeps the per-workgroup pick cheap.
    void enqueue_onesync(uint32_t num_docs, bool few) {
        enqueue_pass0(num_docs, true);
        uint32_t cgrid = few ? 256u
                             : std::min<uint32_t>(2048, (num_docs + 1023) / 1024);
        uint32_t kw = uint32_t(std::min<uint64_t>(leaf_max_hits, 0xFFFFFFFFull));
        launch_cand_pick_compact(wide, cgrid, ctx->stream, d_cand, cand_cap, d_hdr,
                                 d_hist, kw, (uint64_t*)ctx->d_survivors.p,
                                 surv_cap);
        HIP_CHECK(hipMemcpyAsync(ctx->h_topk.p, ctx->d_survivors.p,
                                 size_t(TOPK_INLINE_SURVIVORS) * 8 * rw,
                                 hipMemcpyDeviceToHost, ctx->stream));
        onesync = true;
    }

    // step 3, after the synchronize: `hdr` and `hist` are the downloaded
    // header and pass-0 histogram. Returns through `onesync` whether the
    // survivors are there or select() has to refine from `hist`.
    void onesync_arrived(const uint8_t* hdr, const uint8_t* hist) {
        uint32_t refine, compacted;
        memcpy(&picked_survivors, hdr + TOPK_PICK_COUNT_OFF, 4);
        memcpy(&refine, hdr + TOPK_PICK_REFINE_OFF, 4);
        memcpy(&compacted, hdr + 4, 4);  // cand_hdr_survivors
        hist0 = (uint32_t*)hist;
        hist0_valid = true;
        if (refine) {
            onesync = false;
            ++ctx->topk_onesync_fallbacks;
            return;
        }
        if (compacted != picked_survivors || picked_survivors > surv_cap)
            throw std::runtime_error(
                "top-K one-sync selection: histogram and compaction disagree (" +
                std::to_string(picked_survivors) + " vs " +
                std::to_string(compacted) + ")");
        ++ctx->topk_onesync_calls;
        ctx->topk_onesync_last_survivors = picked_survivors;
        ctx->topk_onesync_last_tail = picked_survivors > TOPK_INLINE_SURVIVORS;
    }

    // step 4: the survivors are in pinned staging, but for a tail beyond the
    // inline records; the same exact sort as the refinement path
    void take_onesync(uint64_t K) {
        const size_t rec = size_t(8) * rw;
        const size_t n = picked_survivors;
        const size_t inl = std::min<size_t>(n, TOPK_INLINE_SURVIVORS);
        top_keys.resize(n * rw);
        memcpy(top_keys.data(), ctx->h_topk.p, inl * rec);
        if (n > inl) {
            ctx->h_topk.ensure((n - inl) * rec);
            HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(ctx->h_topk.p, ctx->d_survivors.p + inl * rec,
                                     (n - inl) * rec, hipMemcpyDeviceToHost,
                                     ctx->stream));
            HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            memcpy(top_keys.data() + inl * rw, ctx->h_topk.p, (n - inl) * rec);
            float tms = 0;
            HIP_CHECK(hipEventElapsedTime(&tms, ctx->ev_start, ctx->ev_stop));
            record_kernel_time(ctx, "topk_select", tms);
        }
        sort_truncate(K);
    }

    // narrow keys: best first, cut to K unless a cursor filter still has to
    // run over them. Keys are distinct (the doc id is part of the key), so
    // sorting only the K best of a longer list gives the same K keys in the
    // same order as sorting all and cutting (1,323 survivors at the 100M
    // flagship: the full sort was ~30 us of the call).
    void sort_truncate(uint64_t K) {
        if (wide) return;
        const bool cut = top_keys.size() > K && !after;
        if (cut && K <= top_keys.size() / 8)  // heap select pays for small K
            std::partial_sort(top_keys.begin(), top_keys.begin() + K,
                              top_keys.end(), std::greater<uint64_t>());
        else
            std::sort(top_keys.begin(), top_keys.end(), std::greater<uint64_t>());
        if (cut) top_keys.resize(K);
    }

    // search_after: pre-compact the band_n candidates to the cursor's
    // primary-value band; selection then runs over the band only
    void compact_cursor_band(uint64_t ceil_key) {
        uint32_t cand_n = uint32_t(band_n);
        qw_ensure_acct(ctx, ctx->d_cand2, size_t(cand_n) * 8 * rw + 16);
        HIP_CHECK(hipMemsetAsync(d_band, 0, 4, ctx->stream));
        uint32_t pgrid = std::min<uint32_t>(2048, (cand_n + 255) / 256);
        launch_cand_compact(wide, pgrid, ctx->stream, d_cand, cand_n, 0ull,
                            ceil_key, (uint64_t*)ctx->d_cand2.p, d_band, cand_n);
        uint32_t n2 = 0;
        HIP_CHECK(hipMemcpyAsync(&n2, d_band, 4, hipMemcpyDeviceToHost,
                                 ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        d_cand = (uint64_t*)ctx->d_cand2.p;
        d_n = d_band;
        band_n = n2;
    }

    // fills top_keys with every record whose key is >= the K-th best key
    void select(uint64_t Kwant) {
        kwant = Kwant;
        const uint32_t cand_n = uint32_t(band_n);
        uint64_t K = std::min<uint64_t>(Kwant, cand_n);
        if (onesync) {
            onesync = false;
            take_onesync(K);
            return;
        }
        uint64_t prefix = 0;
        uint32_t prefix_bits = 0;
        uint64_t survivors = cand_n, above = 0, Krem = K;
        uint64_t floor_key = 0;
        std::vector<uint32_t> hist(TOPK_BINS);
        HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
        while (true) {
            // refine until the band is small: the D2H + host sort of
            // the survivors is on the critical path (a 65k-u64 band
            // cost ~90 us at K=1000; one more 4096-bin pass is ~20 us)
            if (survivors <= std::max<uint64_t>(4 * K, 16384) || prefix_bits >= 48) {
                if (prefix_bits == 0) floor_key = 0;
                break;
            }
            if (prefix_bits == 0 && hist0_valid) {
                memcpy(hist.data(), hist0,
                       TOPK_BINS * 4);  // prefetched with the main sync
            } else {
                HIP_CHECK(hipMemsetAsync(d_hist, 0, TOPK_BINS * 4, ctx->stream));
                // grid small enough that the per-WG 4096-bin LDS flush
                // (global atomics ∝ grid) stays cheap, yet fills the chip
                uint32_t hgrid = std::min<uint32_t>(512, (cand_n + 4095) / 4096);
                launch_cand_hist(wide, hgrid, ctx->stream, d_cand, d_n, prefix,
                                 prefix_bits, d_hist);
                HIP_CHECK(hipMemcpyAsync(hist.data(), d_hist, TOPK_BINS * 4,
                                         hipMemcpyDeviceToHost, ctx->stream));
                HIP_CHECK(hipStreamSynchronize(ctx->stream));
            }
            uint64_t cum = 0;
            int b = TOPK_BINS - 1;
            for (; b >= 0; --b) {
                if (cum + hist[b] >= Krem) break;
                cum += hist[b];
            }
            if (b < 0) b = 0;
            uint32_t shift = 64 - prefix_bits - 12;
            floor_key = (prefix_bits ? (prefix << (64 - prefix_bits)) : 0) |
                        (uint64_t(uint32_t(b)) << shift);
            above += cum;
            survivors = above + hist[b];
            Krem = Krem - cum;
            prefix = (prefix << 12) | uint64_t(uint32_t(b));
            prefix_bits += 12;
        }
        // #keys >= floor_key is known EXACTLY from the histogram walk, so
        // no round trip for the compact count: one async D2H of survivors
        qw_ensure_acct(ctx, ctx->d_survivors, survivors * 8 * rw + 16);
        HIP_CHECK(hipMemsetAsync(d_survivors, 0, 4, ctx->stream));
        uint32_t cgrid = std::min<uint32_t>(2048, (cand_n + 255) / 256);
        launch_cand_compact(wide, cgrid, ctx->stream, d_cand, cand_n, floor_key,
                            ~0ull, (uint64_t*)ctx->d_survivors.p, d_survivors,
                            uint32_t(survivors));
        top_keys.resize(survivors * rw);
        ctx->h_topk.ensure(survivors * 8 * rw + 16);
        HIP_CHECK(hipMemcpyAsync(ctx->h_topk.p, ctx->d_survivors.p,
                                 survivors * 8 * rw, hipMemcpyDeviceToHost,
                                 ctx->stream));
        HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        memcpy(top_keys.data(), ctx->h_topk.p, survivors * 8 * rw);
        float tms = 0;
        HIP_CHECK(hipEventElapsedTime(&tms, ctx->ev_start, ctx->ev_stop));
        record_kernel_time(ctx, "topk_select", tms);
        sort_truncate(K);
    }

    // search_after shortfall: the exact cursor filter left fewer than a page
    // of n_hits hits. Re-selects with K x8 and returns true, or returns
    // false when the page is full or the band is exhausted.
    bool grow(size_t n_hits) {
        if (!after || band_n == 0 ||
            n_hits >= std::min<uint64_t>(leaf_max_hits, band_n) || kwant >= band_n)
            return false;
        select(std::min<uint64_t>(band_n, kwant * 8));
        return true;
    }
};

struct TileRun {
    uint64_t matched = 0;  // sum of the tile counts
    uint32_t cand_n = 0;   // candidate records written
    // downloaded aggregation output (pinned staging), when there are aggs
    const uint8_t* agg_host = nullptr;
};

// query scratch upload + results reset; enqueued before fill_query_dev so
// that host work overlaps the copies
static void enqueue_uploads(qw_ctx* ctx, const ScratchLayout& L,
                            const AggPlan& ap, bool do_aggs) {
    HIP_CHECK(hipMemcpyAsync(ctx->d_scratch.p, ctx->h_scratch.p, L.scratch_bytes,
                             hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(ctx->d_results.p, 0, L.r_agg, ctx->stream));
    if (do_aggs && ap.out_bytes)
        HIP_CHECK(hipMemcpyAsync(ctx->d_results.p + L.r_agg, ap.init.data(),
                                 ap.out_bytes, hipMemcpyHostToDevice, ctx->stream));
}

// the tile kernel, selection pass 0 and every download that rides the same
// synchronize
static TileRun run_leaf_tile(qw_ctx* ctx, const SplitView& sv,
                             const TileLaunch& tl, const ScratchLayout& L,
                             const AggPlan& ap, bool collect, bool do_aggs,
                             TopkSelector& sel, StageTimer& timer) {
    const uint32_t n_tiles = tl.q.n_tiles;
    HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
    launch_leaf_tile(tl.ns, tl.nb, tl.na, collect, dim3(tl.grid), ctx->stream,
                     tl.q, 0u, n_tiles, 1u);
    HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
    HIP_CHECK(hipGetLastError());
    const bool agg_out = do_aggs && ap.out_bytes;
    TileRun run;
    uint32_t* tile_counts;
    uint32_t* pc;
    if (sel.onesync_wanted(collect)) {
        // pass 0, the device pick + compaction and the inline survivors,
        // then ONE download of everything up to the candidate records: tile
        // counts | header | histogram | aggregation output are contiguous
        sel.enqueue_onesync(sv.num_docs, tl.q.prune_k != 0);
        const size_t head = agg_out ? L.r_agg + ap.out_bytes : L.r_agg;
        ctx->h_counts.ensure(head + 64);
        HIP_CHECK(hipMemcpyAsync(ctx->h_counts.p, ctx->d_results.p, head,
                                 hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        tile_counts = (uint32_t*)(ctx->h_counts.p + L.r_tile_counts);
        pc = (uint32_t*)(ctx->h_counts.p + L.r_cand_count);
        run.agg_host = ctx->h_counts.p + L.r_agg;
        sel.onesync_arrived(ctx->h_counts.p + L.r_cand_count,
                            ctx->h_counts.p + L.r_hist);
    } else {
        if (collect && !sel.after) {
            sel.enqueue_pass0(sv.num_docs);
            sel.download_pass0();
        }
        // ---- download counts (into pinned staging: no pageable D2H)
        ctx->h_counts.ensure(size_t(n_tiles) * 4 + 64);
        tile_counts = (uint32_t*)ctx->h_counts.p;
        pc = (uint32_t*)(ctx->h_counts.p + size_t(n_tiles) * 4);
        HIP_CHECK(hipMemcpyAsync(tile_counts, ctx->d_results.p + L.r_tile_counts,
                                 size_t(n_tiles) * 4, hipMemcpyDeviceToHost,
                                 ctx->stream));
        if (collect)
            HIP_CHECK(hipMemcpyAsync(pc, ctx->d_results.p + L.r_cand_count, 4,
                                     hipMemcpyDeviceToHost, ctx->stream));
        if (do_aggs) ctx->h_agg.ensure(ap.out_bytes + 64);
        if (agg_out) {
            // aggregation results ride the same async batch + sync (a
            // blocking copy after hit building cost ~40 us per split)
            HIP_CHECK(hipMemcpyAsync(ctx->h_agg.p, ctx->d_results.p + L.r_agg,
                                     ap.out_bytes, hipMemcpyDeviceToHost,
                                     ctx->stream));
        }
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        run.agg_host = ctx->h_agg.p;
    }
    run.cand_n = collect ? *pc : 0;
    timer.mark("main+pass0+sync");
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
    record_kernel_time(ctx, tl.kname, ms);
    for (uint32_t i = 0; i < n_tiles; ++i) run.matched += tile_counts[i];
    if (collect) {
        ++(tl.q.prune_k ? ctx->topk_pruned : ctx->topk_unpruned);
        ctx->topk_last_emitted = run.cand_n;
        ctx->topk_last_matched = run.matched;
    }
    return run;
}

static pb::PartialHit make_hit(const SplitView& sv, const SortPlan& sp,
                               uint32_t doc, float score) {
    pb::PartialHit h;
    h.split_id = sv.split_id;
    h.segment_ord = sv.segment_ord;
    h.doc_id = doc;
    if (!sp.specs.empty()) h.sort_value = sort_value_of(sp.specs[0], doc, score);
    if (sp.specs.size() > 1) h.sort_value2 = sort_value_of(sp.specs[1], doc, score);
    return h;
}

// PartialHits of the leaf's page, best first
static void build_hits(std::vector<pb::PartialHit>& hits, const SplitView& sv,
                       const SortPlan& sp, bool fq_scoring, TopkSelector& sel,
                       uint64_t leaf_max_hits, bool trivial_hits) {
    if (trivial_hits) {
        // hits enumerable without the kernel: doc-id order (desc default)
        uint64_t k = std::min<uint64_t>(leaf_max_hits, sv.num_docs);
        for (uint64_t i = 0; i < k; ++i) {
            uint32_t doc = sp.order1 == 1 ? uint32_t(sv.num_docs - 1 - i)
                                          : uint32_t(i);
            hits.push_back(make_hit(sv, sp, doc, 0.f));
        }
        return;
    }
    // build hits from the survivors; with search_after, the exact
    // cursor filter runs before truncation and the selection widens
    // (growing K) until the page is full or the band is exhausted
    const std::vector<uint64_t>& top_keys = sel.top_keys;
    do {
        hits.clear();
        hits.reserve(top_keys.size() / (sp.wide ? 2 : 1));
        if (sp.wide) {
            // survivors carry (selection key, score|doc); the exact
            // reference order ((sort_value, sort_value2, GlobalDocId),
            // sorting.md:14-26) is re-established over the survivors
            size_t n = top_keys.size() / 2;
            for (size_t i = 0; i < n; ++i) {
                uint64_t aux = top_keys[2 * i + 1];
                uint32_t doc = uint32_t(aux);
                float score = 0.f;
                if (fq_scoring) {
                    uint32_t b = uint32_t(aux >> 32);
                    memcpy(&score, &b, 4);
                }
                hits.push_back(make_hit(sv, sp, doc, score));
            }
        } else {
            const bool asc = sp.sort_asc();
            for (uint64_t key : top_keys) {
                uint32_t kh = uint32_t(key >> 32), kl = uint32_t(key);
                if (asc) {
                    kh = ~kh;
                    kl = ~kl;
                }
                float score = 0.f;
                if (fq_scoring) {
                    uint32_t b = (kh & 0x80000000u) ? (kh & ~0x80000000u) : ~kh;
                    memcpy(&score, &b, 4);
                }
                hits.push_back(make_hit(sv, sp, kl, score));
            }
        }
        if (sp.after) {
            const bool mixed1 = sp.mixed(0), mixed2 = sp.mixed(1);
            hits.erase(std::remove_if(hits.begin(), hits.end(),
                                      [&](const pb::PartialHit& h) {
                                          return !after_cursor(
                                              h, *sp.after, sp.ck1, sp.ck2,
                                              sp.order1, sp.order2, mixed1,
                                              mixed2);
                                      }),
                       hits.end());
        }
        size_t k = std::min<size_t>(leaf_max_hits, hits.size());
        std::partial_sort(hits.begin(), hits.begin() + k, hits.end(),
                          [&](const pb::PartialHit& a, const pb::PartialHit& b) {
                              return hit_before(a, b, sp.order1, sp.order2);
                          });
        hits.resize(k);
    } while (sel.grow(hits.size()));
}

// one STATS_SLOT_BYTES device stats slot (AggDev::n_sub, gpu_types.h)
static StatsPayload read_stats_slot(const uint8_t* slot) {
    StatsPayload sp;
    uint64_t mn, mx;
    memcpy(&sp.count, slot, 8);
    memcpy(&sp.sum, slot + 8, 8);
    memcpy(&mn, slot + 16, 8);
    memcpy(&mx, slot + 24, 8);
    memcpy(&sp.sum_sq, slot + 32, 8);
    if (sp.count) {
        sp.min = u64_to_f64(mn);
        sp.max = u64_to_f64(mx);
    }
    return sp;
}

// the device output of aggregation i; agg_out is the host copy of the
// results region that starts at r_agg
struct AggOut {
    const AggDef& d;
    const AggDev& a;
    const uint8_t* agg_out;
    size_t r_agg;
    const uint8_t* at(uint64_t results_off) const {
        return agg_out + (results_off - r_agg);
    }
    const uint64_t* counts() const { return (const uint64_t*)at(a.counts_out); }
};

static bool terms_has_perc_sub(const AggDef& d) {
    if (d.kind != AggDef::TERMS) return false;
    for (auto& s : d.sub)
        if (s.kind == MetricAgg::PERCENTILES) return true;
    return false;
}

static void decode_terms(const AggOut& o, const FastFieldView* f,
                         uint64_t matched, AggResult& r) {
    const AggDef& d = o.d;
    const AggDev& a = o.a;
    const uint64_t* counts = o.counts();
    const bool perc_sub = terms_has_perc_sub(d);
    if (perc_sub)
        for (auto& s : d.sub)
            r.sub_kinds.push_back(s.kind == MetricAgg::PERCENTILES ? 1 : 0);
    if (!a.n_buckets) return;
    if (a.nulls_off || a.offsets_off) {
        uint64_t m = 0;
        memcpy(&m, o.at(a.matched_out), 8);
        r.terms_matched_docs = m;
    } else {
        // non-nullable column: every matched doc has a value
        r.terms_matched_docs = matched;
    }
    if (a.kind == AGGD_TERMS_NUM) {
        r.key_kind = f->type == FastFieldView::U64   ? 1
                     : f->type == FastFieldView::F64 ? 3
                                                     : 2;
        uint32_t slots = (a.n_buckets - 2) >> 1;
        if (counts[2 * uint64_t(slots) + 1])
            throw std::runtime_error("numeric terms hash table overflow");
        for (uint64_t s2 = 0; s2 < slots; ++s2) {
            uint64_t key = counts[2 * s2], c = counts[2 * s2 + 1];
            if (key != ~0ull && c)
                r.term_counts.emplace_back(num_term_key(key), c);
        }
        if (uint64_t sc2 = counts[2 * uint64_t(slots)])
            r.term_counts.emplace_back(num_term_key(~0ull), sc2);
        std::sort(r.term_counts.begin(), r.term_counts.end());
    } else {
        const uint8_t* subs = o.at(a.sub_out);
        for (uint32_t ord = 0; ord < a.n_buckets; ++ord) {
            if (!counts[ord]) continue;
            r.term_counts.emplace_back(f->dict_entry(ord), counts[ord]);
            if (!a.n_sub) continue;
            std::vector<StatsPayload> ts(d.sub.size());
            for (uint32_t s = 0; s < a.n_sub; ++s)
                ts[s] = read_stats_slot(
                    subs + (uint64_t(ord) * a.n_sub + s) * STATS_SLOT_BYTES);
            r.term_subs.push_back(std::move(ts));
        }
    }
    if (d.kind == AggDef::TERMS)
        truncate_terms_split(r, effective_split_size(d.size, d.split_size),
                             d.order_target, d.order_asc, &d.sub);
    // the kept rows, empty until terms_perc_pass fills them in this order
    if (perc_sub)
        r.term_sketches.assign(r.term_counts.size(),
                               std::vector<SketchPayload>(d.sub.size()));
}

// decode packed 63-bit keys into the canonical per-source byte encoding
// (split-local ords -> term strings) so the cross-split QAGG merge compares
// composite tuples directly
static void decode_composite(
    const AggOut& o, const std::array<const FastFieldView*, 4>& fields,
    const std::array<uint32_t, 4>& width, AggResult& r) {
    const AggDef& d = o.d;
    const AggDev& a = o.a;
    const uint64_t* counts = o.counts();
    r.key_kind = 9;
    if (!a.n_buckets) return;
    uint32_t slots = (a.n_buckets - 2) >> 1;
    if (counts[2 * uint64_t(slots) + 1])
        throw std::runtime_error("composite hash table overflow");
    for (uint64_t s2 = 0; s2 < slots; ++s2) {
        uint64_t key = counts[2 * s2], c = counts[2 * s2 + 1];
        if (key == ~0ull || !c) continue;
        std::string ck;
        for (size_t si = 0; si < d.comp.size(); ++si) {
            const CompSource& cs = d.comp[si];
            uint64_t comp = (key >> a.c_shift[si]) & ((1ull << width[si]) - 1);
            uint64_t miss = cs.missing_bucket ? 1 : 0;
            if (miss && comp == 0) {
                comp_encode_null(ck);
            } else if (cs.is_histo) {
                double v = double(a.c_base[si] + int64_t(comp - miss)) *
                               cs.interval +
                           cs.offset;
                comp_encode_f64(ck, v);
            } else {
                comp_encode_str(ck, fields[si]->dict_entry(uint32_t(comp - miss)));
            }
        }
        r.term_counts.emplace_back(std::move(ck), c);
    }
    std::sort(r.term_counts.begin(), r.term_counts.end());
}

static void decode_histogram(const AggOut& o, AggResult& r) {
    const AggDef& d = o.d;
    const AggDev& a = o.a;
    const uint64_t* counts = o.counts();
    for (auto& sdef : d.sub)
        r.sub_kinds.push_back(sdef.kind == MetricAgg::PERCENTILES ? 1 : 0);
    const uint8_t* subs = o.at(a.sub_out);
    const uint64_t* pwords =
        a.p_si != 0xFF ? (const uint64_t*)o.at(a.p_out) : nullptr;
    for (uint32_t bi = 0; bi < a.n_buckets; ++bi) {
        if (!counts[bi]) continue;
        AggBucket b;
        b.key = double(a.base_index + int64_t(bi)) * d.interval + d.offset;
        b.doc_count = counts[bi];
        b.sub.resize(d.sub.size());
        b.psub.resize(d.sub.size());
        if (pwords) {
            const uint64_t* pw = pwords + uint64_t(bi) * (a.p_n_keys + 1);
            SketchPayload& pp = b.psub[a.p_si];
            pp.zero = pw[0];
            for (uint32_t j = 1; j <= a.p_n_keys; ++j)
                if (pw[j]) pp.counts[a.p_k_lo + int32_t(j) - 1] = pw[j];
        }
        for (uint32_t s = 0; s < a.n_sub; ++s) {
            if (s == a.p_si) continue;
            b.sub[s] = read_stats_slot(
                subs + (uint64_t(bi) * a.n_sub + s) * STATS_SLOT_BYTES);
        }
        r.buckets.push_back(std::move(b));
    }
}

// aggregation assembly (QAGG1 intermediate) from the downloaded results
static void decode_aggs(const AggPlan& ap, size_t r_agg, const uint8_t* agg_out,
                        uint64_t matched, IntermediateAggResults& out) {
    for (size_t i = 0; i < ap.defs.size(); ++i) {
        const AggDef& d = ap.defs[i];
        const AggDev& a = ap.devs[i];
        const AggOut o{d, a, agg_out, r_agg};
        AggResult r;
        r.name = d.name;
        r.kind = agg_result_kind(d);
        for (auto& s : d.sub) r.sub_names.push_back(s.name);
        switch (r.kind) {
            case 3:
                if (d.kind == AggDef::COMPOSITE)
                    decode_composite(o, ap.comp_fields[i], ap.comp_width[i], r);
                else decode_terms(o, ap.fields[i], matched, r);
                break;
            case 6:
                if (a.n_buckets) {
                    const uint64_t* counts = o.counts();
                    r.sketch.zero = counts[0];
                    for (uint32_t j = 1; j < a.n_buckets; ++j)
                        if (counts[j])
                            r.sketch.counts[a.p_k_lo + int32_t(j) - 1] = counts[j];
                }
                break;
            case 5:
                if (a.n_buckets) r.metric = read_stats_slot(o.at(a.counts_out));
                break;
            case 4:
                for (uint32_t ri = 0; ri < a.n_buckets; ++ri) {
                    if (!o.counts()[ri]) continue;
                    AggBucket b;
                    b.key = double(ri);  // range index; finalize maps back
                    b.doc_count = o.counts()[ri];
                    r.buckets.push_back(std::move(b));
                }
                break;
            default:
                decode_histogram(o, r);
        }
        out.aggs.push_back(std::move(r));
    }
}

// device buffers of one terms_perc_pass: the same holder as the gate
// bitmaps, counted in hbm_used while they live and freed on whatever exit
using PassBufs = GateBitmaps;

// Percentiles under terms: the tile kernel counted every
// ordinal and decode_terms cut the result to the kept terms; this second pass
// sketches the sub values of those kept buckets only, over the match set of
// the same plan (bitmap_eval: every predicate of pass 1, no search_after).
static void terms_perc_pass(qw_ctx* ctx, const DeviceSplit& ds,
                            const PlanNode& plan, const Schema& schema,
                            const AggPlan& ap, uint64_t matched,
                            IntermediateAggResults& out) {
    const SplitView& sv = ds.view;
    struct Sub {
        size_t si;
        const FastFieldView* sf;
        int32_t k_lo;
        std::vector<double> bounds;
    };
    for (size_t i = 0; i < ap.defs.size(); ++i) {
        const AggDef& d = ap.defs[i];
        const AggDev& a = ap.devs[i];
        const FastFieldView* f = ap.fields[i];
        AggResult& r = out.aggs[i];
        if (!terms_has_perc_sub(d) || a.kind != AGGD_TERMS || !a.n_buckets)
            continue;
        const size_t kept = r.term_counts.size();
        if (!kept || !matched) continue;

        std::vector<Sub> subs;
        for (size_t si = 0; si < d.sub.size(); ++si) {
            if (d.sub[si].kind != MetricAgg::PERCENTILES) continue;
            const FastFieldView* sf = sv.fast_field(d.sub[si].field);
            // missing, str or multi-valued column: the sketches stay empty
            if (!sf || sf->type == FastFieldView::STR || sf->multi) continue;
            double mn, mx;
            col_min_max(*sf, &mn, &mx);
            int32_t k_lo = 0, k_hi = 0;
            if (mx >= PERC_MIN_VALUE) {
                k_lo = perc_key_for(std::max(mn, PERC_MIN_VALUE));
                k_hi = perc_key_for(mx);
            }
            Sub s{si, sf, k_lo, {}};
            if (uint64_t(kept) * (uint64_t(k_hi - k_lo + 1) + 1) > (1ull << 25))
                throw std::runtime_error(
                    "percentiles sketch region too large (r1 limit)");
            perc_boundaries(k_lo, k_hi, s.bounds);
            subs.push_back(std::move(s));
        }
        if (subs.empty()) continue;

        const uint8_t* bm = bitmap_eval(ctx, ds, plan, schema);
        PassBufs bufs(ctx);
        // kept terms are in key order = ordinal order
        std::vector<uint32_t> remap(f->cardinality, TERMS_PERC_UNKEPT);
        for (size_t t = 0; t < kept; ++t) {
            uint32_t ord = f->str_bound_ord(r.term_counts[t].first, false);
            if (ord >= f->cardinality)
                throw std::runtime_error("terms percentiles: kept term not in "
                                         "the dictionary");
            remap[ord] = uint32_t(t);
        }
        uint32_t* d_remap = (uint32_t*)bufs.alloc(remap.size() * 4);
        HIP_CHECK(hipMemcpyAsync(d_remap, remap.data(), remap.size() * 4,
                                 hipMemcpyHostToDevice, ctx->stream));
        for (const Sub& s : subs) {
            const uint32_t n_keys = uint32_t(s.bounds.size());
            const size_t words = kept * (size_t(n_keys) + 1);
            double* d_bounds = (double*)bufs.alloc(size_t(n_keys) * 8);
            uint64_t* d_out = (uint64_t*)bufs.alloc(words * 8);
            HIP_CHECK(hipMemcpyAsync(d_bounds, s.bounds.data(),
                                     size_t(n_keys) * 8, hipMemcpyHostToDevice,
                                     ctx->stream));
            HIP_CHECK(hipMemsetAsync(d_out, 0, words * 8, ctx->stream));
            TermsPercDev p{};
            p.split = ds.d_image;
            p.bitmap = (const uint32_t*)bm;
            p.remap = d_remap;
            p.bounds = d_bounds;
            p.out = d_out;
            p.num_docs = sv.num_docs;
            p.cardinality = f->cardinality;
            p.kept = uint32_t(kept);
            p.n_keys = n_keys;
            p.ord_off = a.values_off;
            p.ord_nulls_off = a.nulls_off;
            p.ord_offsets_off = a.offsets_off;
            p.ord_width = a.value_width;
            p.val_kind = s.sf->type == FastFieldView::U64   ? 0
                         : s.sf->type == FastFieldView::F64 ? 2
                                                            : 1;
            p.val_off = s.sf->values.off;
            p.val_nulls_off = s.sf->nullable ? s.sf->nulls.off : 0;
            // LDS rule: the table when it fits half the
            // block's budget, the counters when they fit what is left
            size_t lds = 0;
            if (size_t(n_keys) * 8 <= TERMS_PERC_LDS_BYTES / 2) {
                p.lds_bounds = 1;
                lds = size_t(n_keys) * 8;
            }
            if (lds + words * 4 <= TERMS_PERC_LDS_BYTES) {
                p.lds_sketch = 1;
                lds += words * 4;
            }
            // a block with LDS counters pays a zeroing and a flush of the
            // whole region, so fewer, longer blocks: 512 = two for each of
            // the MI355X's 256 CUs; without LDS counters 2048, as the other
            // grid-stride kernels here use. Neither cap has been tuned.
            uint32_t chunks = (sv.num_docs + 255u) / 256u;
            uint32_t grid = std::min<uint32_t>(p.lds_sketch ? 512u : 2048u,
                                               std::max<uint32_t>(chunks, 1u));
            HIP_CHECK(hipEventRecord(ctx->ev_start, ctx->stream));
            launch_terms_perc_sketch(p, grid, uint32_t(lds), ctx->stream);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipEventRecord(ctx->ev_stop, ctx->stream));
            std::vector<uint64_t> host(words);
            HIP_CHECK(hipMemcpyAsync(host.data(), d_out, words * 8,
                                     hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_start, ctx->ev_stop));
            record_kernel_time(ctx, "k_terms_perc_sketch", ms);
            for (size_t t = 0; t < kept; ++t) {
                const uint64_t* pw = host.data() + t * (size_t(n_keys) + 1);
                SketchPayload& pp = r.term_sketches[t][s.si];
                pp.zero = pw[0];
                for (uint32_t j = 1; j <= n_keys; ++j)
                    if (pw[j]) pp.counts[s.k_lo + int32_t(j) - 1] = pw[j];
            }
        }
    }
}

static SplitResult search_split_gpu(qw_ctx* ctx, const DeviceSplit& ds,
                                    const pb::SearchRequest& req, const Schema& schema) {
    SplitResult out;
    StageTimer timer;
    const SplitView& sv = ds.view;
    ctx->hitsets.begin_query();  // unpin previous query's bitmap entries

    PlanNode plan = leaf_plan(ctx, sv, req, schema);
    SortPlan sp = make_sort_plan(sv, req);
    GateBitmaps gate_tmp(ctx);  // outlives every launch below
    FlatQuery fq = flatten_or_bitmap(ctx, ds, plan, schema, sp.scoring, gate_tmp);
    // report required terms flattening proved absent; the caller inserts
    // into the absence cache (for multi-segment splits only terms absent
    // from EVERY segment qualify)
    out.absent_required = fq.absent_required;
    const uint64_t leaf_max_hits = req.max_hits + req.start_offset;
    const bool do_aggs = req.aggregation_request.has_value();

    if (fq.match_none || sv.num_docs == 0) {
        if (do_aggs) {
            empty_agg_shapes(*req.aggregation_request, out.aggs);
            out.has_aggs = true;
        }
        out.micros = timer.micros();
        return out;
    }

    const uint32_t n_tiles = (sv.num_docs + TILE_DOCS - 1) / TILE_DOCS;
    const bool pure_match_all =
        fq.match_all && fq.preds.empty() && fq.terms.empty();
    // hits trivially enumerable only under doc-id order (leaf.rs default)
    const bool trivial_hits = pure_match_all && sp.specs.empty() && !sp.after;
    // candidate collection: needed unless hits are trivially enumerable
    const bool collect = leaf_max_hits > 0 && !trivial_hits && !fq.match_none;
    const bool need_kernel = !pure_match_all || do_aggs || collect;

    // ---- scratch assembly (descriptors + ktabs + block ranges), one H2D
    TermTables tt = build_term_tables(sv, fq);
    ScratchLayout L = layout_results_head(n_tiles);
    AggPlan ap;
    if (do_aggs)
        ap = plan_aggs(sv, *req.aggregation_request, ctx->agg_bucket_limit,
                       L.r_agg);
    layout_finish(L, tt, fq, ap, collect ? sv.num_docs : 0, sp.wide);
    eager_pred_flags(sv, fq);
    timer.mark("plan");
    // per-term block ranges come from the split-level device cache
    // (term_ranges_addr): first query pays the walk+upload, repeats don't
    ctx->h_scratch.ensure(L.scratch_bytes);
    for (size_t i = 0; i < fq.terms.size(); ++i) {
        const FlatQuery::FTerm& t = fq.terms[i];
        tt.terms[i].ranges_addr =
            term_ranges_addr(ctx, ds, t.f, t.tid, n_tiles, sv.num_docs);
    }
    timer.mark("ranges");
    assemble_scratch(ctx->h_scratch.p, L, tt, fq, ap);
    timer.mark("assembly");

    uint64_t matched = sv.num_docs;  // pure match_all, no aggs: no kernel
    const uint8_t* agg_host = nullptr;  // do_aggs always runs the kernel
    TopkSelector sel(ctx, sp.wide, sp.after != nullptr, leaf_max_hits);
    if (need_kernel) {
        qw_ensure_acct(ctx, ctx->d_scratch, L.scratch_bytes);
        qw_ensure_acct(ctx, ctx->d_results, L.results_bytes);
        sel.attach(L);
        if (sel.onesync_wanted(collect)) sel.reserve_onesync(sv.num_docs);
        enqueue_uploads(ctx, L, ap, do_aggs);
        TileLaunch tl = fill_query_dev(ctx, ds, fq, sp, tt, ap, L, collect,
                                       do_aggs, leaf_max_hits, n_tiles);
        TileRun run = run_leaf_tile(ctx, sv, tl, L, ap, collect, do_aggs, sel, timer);
        matched = run.matched;
        agg_host = run.agg_host;
        if (collect && run.cand_n > 0) {
            sel.band_n = run.cand_n;
            if (sp.after) sel.compact_cursor_band(cursor_ceil_key(sp, fq.scoring));
            if (sel.band_n > 0) {
                sel.select(std::min<uint64_t>(
                    leaf_max_hits + (sp.after ? 1024 : 0), sel.band_n));
                timer.mark("topk_select");
            }
        }
    }
    if (pure_match_all) matched = sv.num_docs;
    out.num_hits = matched;

    if (leaf_max_hits > 0)
        build_hits(out.hits, sv, sp, fq.scoring, sel, leaf_max_hits, trivial_hits);
    timer.mark("build_hits");

    if (do_aggs) {
        // downloaded asynchronously with the counts batch (pinned)
        decode_aggs(ap, L.r_agg, agg_host, matched, out.aggs);
        out.has_aggs = true;
    }
    timer.mark("aggs_assembly");
    if (do_aggs) {
        // last: its bitmap evaluation reuses the scratch and results buffers
        terms_perc_pass(ctx, ds, plan, schema, ap, matched, out.aggs);
        timer.mark("terms_perc_pass");
    }

    out.micros = timer.micros();
    return out;
}

// ------------------------------------------------------------ pruning
// Restates CanSplitDoBetter (leaf.rs:1337-1553), simplify_search_request
// (leaf.rs:1666-1710) and the request-level part of rewrite_request
// (leaf.rs:977-990, remove_redundant_timestamp_range :1106-1211). The
// FindTraceIdsAggregation variant (Jaeger traces) is out of scope.
// Missing split timestamps read as 0 (prost's Option accessor default, the
// exact behavior of split.timestamp_start()/timestamp_end() in the reference).
// one split = one or more segments (collector.rs:475-594 per-segment
// collection): run the per-segment search and merge within the split with
// the exact (sort_value, sort_value2, split, segment_ord, doc) order
static SplitResult search_device_split(qw_ctx* ctx, const DeviceSplit& ds,
                                       const pb::SearchRequest& req,
                                       const Schema& schema) {
    using namespace qw;
    std::vector<const DeviceSplit*> segs;
    if (ds.segs.empty()) segs.push_back(&ds);
    else
        for (auto& sp : ds.segs) segs.push_back(sp.get());
    SplitResult out;
    std::map<std::pair<std::string, std::string>, size_t> absent;
    for (const DeviceSplit* seg : segs) {
        SplitResult r = search_split_gpu(ctx, *seg, req, schema);
        out.num_hits += r.num_hits;
        for (auto& h : r.hits) out.hits.push_back(std::move(h));
        if (r.has_aggs) {
            if (!out.has_aggs) {
                out.aggs = std::move(r.aggs);
                out.has_aggs = true;
            } else out.aggs.merge(r.aggs);
        }
        out.micros += r.micros;
        for (auto& ab : r.absent_required) absent[ab]++;
    }
    // absence cache: only terms absent from EVERY segment of the split
    // qualify (the reference early-aborts when warmup finds the term in no
    // segment, leaf.rs:315-320)
    const std::string& sid = segs[0]->view.split_id;
    for (auto& kv : absent)
        if (kv.second == segs.size() &&
            ctx->absence.keys.size() < ctx->absence.cap)
            ctx->absence.keys.insert(
                AbsenceCache::key(sid, kv.first.first, kv.first.second));
    uint64_t leaf_max = req.max_hits + req.start_offset;
    if (segs.size() > 1 && leaf_max > 0 && !out.hits.empty()) {
        int order1, order2;
        request_sort_orders(req, &order1, &order2);
        size_t k = std::min<uint64_t>(leaf_max, out.hits.size());
        std::partial_sort(out.hits.begin(), out.hits.begin() + k,
                          out.hits.end(),
                          [&](const pb::PartialHit& a, const pb::PartialHit& b) {
                              return hit_before(a, b, order1, order2);
                          });
        out.hits.resize(k);
    }
    return out;
}

static int64_t split_ts_start(const pb::SplitIdAndFooterOffsets& s) {
    return s.timestamp_start ? *s.timestamp_start : 0;
}
static int64_t split_ts_end(const pb::SplitIdAndFooterOffsets& s) {
    return s.timestamp_end ? *s.timestamp_end : 0;
}

static int64_t div_ceil_i64(int64_t lhs, int64_t rhs) {  // quickwit-common lib.rs:210
    int64_t d = lhs / rhs, r = lhs % rhs;
    return ((r > 0 && rhs > 0) || (r < 0 && rhs < 0)) ? d + 1 : d;
}

struct SplitFilter {
    enum Kind { UNINFORMATIVE, SPLIT_ID_HIGHER, TS_HIGHER, TS_LOWER } kind =
        UNINFORMATIVE;
    bool has = false;     // a worst-of-top-K hit has been recorded
    std::string wid;      // SPLIT_ID_HIGHER: worst split id
    int64_t wts = 0;      // TS_*: worst timestamp in seconds

    static SplitFilter from_request(const pb::SearchRequest& req,
                                    const std::string& ts_field) {
        SplitFilter f;
        if (req.sort_fields.empty()) {
            f.kind = SPLIT_ID_HIGHER;
        } else if (!ts_field.empty() && req.sort_fields[0].field_name == ts_field) {
            f.kind = req.sort_fields[0].sort_order == 1 ? TS_HIGHER : TS_LOWER;
        }
        return f;
    }

    bool can_be_better(const pb::SplitIdAndFooterOffsets& s) const {
        if (!has) return true;
        switch (kind) {
            case SPLIT_ID_HIGHER: return s.split_id >= wid;
            case TS_HIGHER: return split_ts_end(s) >= wts;
            case TS_LOWER: return split_ts_start(s) <= wts;
            default: return true;
        }
    }

    // record the worst of the (now full) top-K (leaf.rs:1516-1542)
    void record_new_worst_hit(const pb::PartialHit& h) {
        switch (kind) {
            case SPLIT_ID_HIGHER:
                has = true;
                wid = h.split_id;
                break;
            case TS_HIGHER:
                if (h.sort_value.kind == pb::SortByValue::I64) {
                    has = true;
                    wts = div_ceil_i64(h.sort_value.i64, 1000000000);  // round UP
                }
                break;
            case TS_LOWER:
                if (h.sort_value.kind == pb::SortByValue::I64) {
                    has = true;
                    wts = h.sort_value.i64 / 1000000000;  // truncate (Rust /)
                }
                break;
            default: break;
        }
    }
};

static bool is_simple_all_query(const pb::SearchRequest& r) {  // leaf.rs:1315
    if (r.aggregation_request) return false;
    if (r.search_after) return false;
    if (r.start_timestamp || r.end_timestamp) return false;
    try {
        mj::ValuePtr v = mj::parse(r.query_ast);
        const mj::Value* t = v->get("type");
        return t && t->kind == mj::Value::STR && t->s == "match_all";
    } catch (...) {
        return false;
    }
}

static void disable_search_request_hits(pb::SearchRequest& r) {  // leaf.rs:1705
    r.max_hits = 0;
    r.start_offset = 0;
    r.sort_fields.clear();
    r.search_after.reset();
}

}  // namespace qw

// ============================================================== C ABI
static thread_local std::string g_tls_error;

static void set_err(qw_ctx* ctx, const std::string& msg) {
    if (ctx) ctx->last_error = msg;
    else g_tls_error = msg;
}

static void fill_buf(qw_buf* out, const std::string& s) {
    out->data = (uint8_t*)malloc(s.size() ? s.size() : 1);
    memcpy(out->data, s.data(), s.size());
    out->len = s.size();
}

extern "C" {

const char* qw_version(void) { return "quickwit_amd 0.1 gfx950"; }

qw_ctx* qw_ctx_create(const char* config_json) {
    auto* ctx = new qw_ctx();
    try {
        if (config_json && *config_json) {
            mj::ValuePtr cfg = mj::parse(config_json);
            if (const mj::Value* d = cfg->get("device")) ctx->device = int(d->as_i64());
            if (const mj::Value* b = cfg->get("aggregation_bucket_limit"))
                ctx->agg_bucket_limit = b->as_i64();
            if (const mj::Value* c = cfg->get("partial_request_cache_capacity"))
                ctx->leaf_cache.capacity = size_t(c->as_i64());
            if (const mj::Value* mb = cfg->get("hbm_memory_budget")) {
                ctx->hbm_budget = uint64_t(mb->as_i64());
                ctx->budget_configured = true;
            }
            if (const mj::Value* tp = cfg->get("topk_prune"))
                ctx->topk_prune = tp->kind == mj::Value::BOOL ? tp->b
                                                              : tp->as_i64() != 0;
            if (const mj::Value* os = cfg->get("topk_onesync"))
                ctx->topk_onesync = os->kind == mj::Value::BOOL ? os->b
                                                                : os->as_i64() != 0;
        }
        return ctx;
    } catch (const std::exception& e) {
        g_tls_error = e.what();
        delete ctx;
        return nullptr;
    }
}

void qw_ctx_free(qw_ctx* ctx) {
    if (!ctx) return;
    if (ctx->device_ready) {
        (void)hipSetDevice(ctx->device);
        for (auto& kv : ctx->splits) {
            kv.second->free_range_cache();
            for (auto& sg : kv.second->segs) sg->free_range_cache();
            if (kv.second->d_image) (void)hipFree(kv.second->d_image);
        }
        ctx->hitsets.clear();
        if (ctx->ev_start) (void)hipEventDestroy(ctx->ev_start);
        if (ctx->ev_stop) (void)hipEventDestroy(ctx->ev_stop);
        if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    }
    delete ctx;
}

const char* qw_last_error(const qw_ctx* ctx) {
    return ctx ? ctx->last_error.c_str() : g_tls_error.c_str();
}

int32_t qw_ctx_add_split(qw_ctx* ctx, const char* split_id, const uint8_t* data,
                         size_t len) {
    using namespace qw;
    try {
        ctx_ensure_device(ctx);
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_NO_GPU;
    }
    try {
        auto ds = std::make_unique<DeviceSplit>();
        ds->host.assign(data, data + len);
        if (len >= 88 && memcmp(data, "QWAMDSP2", 8) == 0) {
            // QWA2 multi-segment container: outer meta lists per-segment
            // QWA1 images; children alias the parent host/device image
            if (memcmp(data + len - 8, "QWA1FOOT", 8) != 0)
                throw std::runtime_error("bad QWA2 footer");
            uint64_t moff, mlen;
            memcpy(&moff, data + len - 24, 8);
            memcpy(&mlen, data + len - 16, 8);
            if (moff + mlen > len) throw std::runtime_error("bad QWA2 footer");
            mj::ValuePtr meta = mj::parse((const char*)data + moff, mlen);
            uint32_t ord = 0;
            for (auto& sgv : meta->at("segments")->arr) {
                uint64_t off = uint64_t(sgv->at("off")->as_i64());
                uint64_t slen = uint64_t(sgv->at("len")->as_i64());
                if (off + slen > len)
                    throw std::runtime_error("QWA2: segment out of bounds");
                auto child = std::make_unique<DeviceSplit>();
                child->owns_image = false;
                child->view.parse(ds->host.data() + off, slen);
                if (child->view.version < 2)
                    throw std::runtime_error("QWA2 segment: v1 container");
                child->view.split_id = split_id;
                child->view.segment_ord = ord++;
                child->len = slen;
                child->total_docs = child->view.num_docs;
                ds->total_docs += child->view.num_docs;
                ds->segs.push_back(std::move(child));
            }
            if (ds->segs.empty())
                throw std::runtime_error("QWA2: no segments");
            ds->view = ds->segs[0]->view;  // pointers alias ds->host
        } else {
            ds->view.parse(ds->host.data(), len);
            // the caller's split id is authoritative (the request names
            // splits by SplitIdAndFooterOffsets.split_id and the response
            // must echo it); the container's own id is only a default
            ds->view.split_id = split_id;
            if (ds->view.version < 2)
                throw std::runtime_error(
                    "QWA1 v1 container lacks posting segment anchors "
                    "(regenerate the split with the current writer)");
            ds->total_docs = ds->view.num_docs;
        }
        ds->len = len;
        HIP_CHECK(hipSetDevice(ctx->device));
        try {
            qw_check_budget(ctx, len + 64);
        } catch (const std::exception& e) {
            set_err(ctx, e.what());
            return QW_ERR_OVER_MEMORY_BUDGET;
        }
        HIP_CHECK(hipMalloc(&ds->d_image, len + 64));  // +64: decode overread pad
        HIP_CHECK(hipMemcpy(ds->d_image, data, len, hipMemcpyHostToDevice));
        ctx->hbm_used += len + 64;
        {
            // children point into the parent device image (their views'
            // offsets are relative to their own segment base)
            size_t ci = 0;
            uint64_t moff2, mlen2;
            if (!ds->segs.empty()) {
                mj::ValuePtr meta2;
                memcpy(&moff2, data + len - 24, 8);
                memcpy(&mlen2, data + len - 16, 8);
                meta2 = mj::parse((const char*)data + moff2, mlen2);
                for (auto& sgv : meta2->at("segments")->arr)
                    ds->segs[ci++]->d_image =
                        ds->d_image + uint64_t(sgv->at("off")->as_i64());
            }
        }
        ctx->splits[split_id] = std::move(ds);
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_BAD_SPLIT;
    }
}

int32_t qw_ctx_remove_split(qw_ctx* ctx, const char* split_id) {
    auto it = ctx->splits.find(split_id);
    if (it == ctx->splits.end()) return QW_ERR_NOT_FOUND;
    ctx->hbm_used -= it->second->range_cache_bytes;
    it->second->free_range_cache();
    for (auto& sg : it->second->segs) {
        ctx->hbm_used -= sg->range_cache_bytes;
        sg->free_range_cache();
    }
    if (it->second->d_image) {
        (void)hipFree(it->second->d_image);
        ctx->hbm_used -= it->second->len + 64;
    }
    ctx->splits.erase(it);
    ctx->leaf_cache.remove_split(split_id);
    ctx->hitsets.remove_split(split_id);
    ctx->absence.remove_split(split_id);
    return QW_OK;
}

int32_t qw_leaf_search(qw_ctx* ctx, const uint8_t* req_pb, size_t req_len,
                       qw_buf* out) {
    using namespace qw;
    try {
        ctx_ensure_device(ctx);
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_NO_GPU;
    }
    try {
        HIP_CHECK(hipSetDevice(ctx->device));
        pb::LeafSearchRequest lreq = pb::LeafSearchRequest::decode(req_pb, req_len);
        const pb::SearchRequest& req = lreq.search_request;
        if (lreq.doc_mappers.empty()) throw std::runtime_error("missing doc_mapper");
        Schema schema = Schema::parse(lreq.doc_mappers[0]);

        struct Task {
            pb::SplitIdAndFooterOffsets so;
            const DeviceSplit* ds;
            pb::SearchRequest req;  // per-split request (may be demoted)
        };
        std::vector<Task> tasks;
        std::vector<pb::SplitSearchError> pre_failed;
        for (auto& lr : lreq.leaf_requests)
            for (auto& so : lr.split_offsets) {
                auto it = ctx->splits.find(so.split_id);
                if (it == ctx->splits.end()) {
                    // a split that cannot be opened is a per-split failure
                    // inside the response (leaf.rs:2143-2148), not a
                    // whole-call error — the other splits still answer
                    pb::SplitSearchError se;
                    se.error = "unknown split: " + so.split_id;
                    se.split_id = so.split_id;
                    se.retryable_error = true;
                    pre_failed.push_back(std::move(se));
                    continue;
                }
                tasks.push_back({so, it->second.get(), req});
            }

        // ---- pruning: split ordering + upfront count-only demotion
        // (CanSplitDoBetter::optimize, leaf.rs:1403-1514)
        SplitFilter filter = SplitFilter::from_request(req, schema.timestamp_field);
        switch (filter.kind) {
            case SplitFilter::SPLIT_ID_HIGHER:
                std::sort(tasks.begin(), tasks.end(), [](const Task& a, const Task& b) {
                    return b.so.split_id < a.so.split_id;
                });
                break;
            case SplitFilter::TS_HIGHER:
                std::sort(tasks.begin(), tasks.end(), [](const Task& a, const Task& b) {
                    return split_ts_end(b.so) < split_ts_end(a.so);
                });
                break;
            case SplitFilter::TS_LOWER:
                std::sort(tasks.begin(), tasks.end(), [](const Task& a, const Task& b) {
                    return split_ts_start(a.so) < split_ts_start(b.so);
                });
                break;
            default: break;
        }
        if (is_simple_all_query(req)) {
            uint64_t num_requested = req.start_offset + req.max_hits;
            size_t mrs = 0;  // number of splits guaranteed to fill the top-K
            uint64_t psum = 0;
            for (const Task& t : tasks) {
                psum += t.so.num_docs;
                if (psum >= num_requested) break;
                ++mrs;
            }
            mrs += 1;
            if (filter.kind == SplitFilter::SPLIT_ID_HIGHER) {
                for (size_t i = mrs; i < tasks.size(); ++i)
                    disable_search_request_hits(tasks[i].req);
            } else if (filter.kind == SplitFilter::TS_LOWER) {
                int64_t biggest_end = INT64_MIN;
                for (size_t i = 0; i < std::min(mrs, tasks.size()); ++i)
                    biggest_end = std::max(biggest_end, split_ts_end(tasks[i].so));
                for (size_t i = mrs; i < tasks.size(); ++i)
                    if (split_ts_start(tasks[i].so) > biggest_end)
                        disable_search_request_hits(tasks[i].req);
            } else if (filter.kind == SplitFilter::TS_HIGHER) {
                int64_t smallest_start = INT64_MAX;
                for (size_t i = 0; i < std::min(mrs, tasks.size()); ++i)
                    smallest_start = std::min(smallest_start, split_ts_start(tasks[i].so));
                for (size_t i = mrs; i < tasks.size(); ++i)
                    if (split_ts_end(tasks[i].so) < smallest_start)
                        disable_search_request_hits(tasks[i].req);
            }
        }
        // per-split rewrite (leaf.rs:977-990): drop sort fields on count-only
        // requests; drop request-level ts bounds covered by the split range
        for (Task& t : tasks) {
            if (t.req.max_hits == 0) t.req.sort_fields.clear();
            if (!schema.timestamp_field.empty()) {
                if (t.req.start_timestamp && t.so.timestamp_start &&
                    *t.req.start_timestamp <= *t.so.timestamp_start)
                    t.req.start_timestamp.reset();
                if (t.req.end_timestamp && t.so.timestamp_end &&
                    *t.req.end_timestamp >= *t.so.timestamp_end + 1)
                    t.req.end_timestamp.reset();
            }
        }

        pb::LeafSearchResponse resp;
        for (auto& se : pre_failed) {
            resp.num_attempted_splits++;
            resp.failed_splits.push_back(std::move(se));
        }
        IntermediateAggResults merged_aggs;
        bool any_aggs = false;
        std::vector<pb::PartialHit> all_hits;
        pb::LeafResourceStats rstats;
        rstats.search_pool_cpu_threads = 1;  // one host thread per GPU
        uint64_t worst = 0;
        int order1 = req.sort_fields.empty() ? 1 : req.sort_fields[0].sort_order;
        int order2 = req.sort_fields.size() > 1 ? req.sort_fields[1].sort_order : 1;
        auto cmp = [&](const pb::PartialHit& a, const pb::PartialHit& b) {
            return hit_before(a, b, order1, order2);
        };
        uint64_t leaf_max = req.max_hits + req.start_offset;
        for (Task& t : tasks) {
            // second simplify pass against the live filter state
            // (simplify_search_request, leaf.rs:1666-1703)
            if (!filter.can_be_better(t.so)) disable_search_request_hits(t.req);
            if (t.req.max_hits == 0 && !t.req.aggregation_request &&
                t.req.count_hits != 0 /* != CountHits::CountAll */)
                continue;  // pruned before warmup — not attempted
            resp.num_attempted_splits++;
            // partial-result cache probe (leaf.rs:667 / leaf_cache.rs)
            std::string ckey;
            bool cacheable = ctx->leaf_cache.capacity > 0;
            if (cacheable) {
                ckey = leaf_cache_key(t.so, t.req);
                std::string hit;
                if (ctx->leaf_cache.get(ckey, &hit)) {
                    pb::LeafSearchResponse cr = pb::LeafSearchResponse::decode(
                        (const uint8_t*)hit.data(), hit.size());
                    resp.num_successful_splits++;
                    resp.num_hits += cr.num_hits;
                    for (auto& h : cr.partial_hits) all_hits.push_back(std::move(h));
                    if (cr.intermediate_aggregation_result) {
                        IntermediateAggResults ir = IntermediateAggResults::decode(
                            (const uint8_t*)cr.intermediate_aggregation_result->data(),
                            cr.intermediate_aggregation_result->size());
                        if (!any_aggs) {
                            merged_aggs = std::move(ir);
                            any_aggs = true;
                        } else merged_aggs.merge(ir);
                    }
                    // cache-hit stats (leaf_cache.rs:73-79 overwrite-on-put)
                    rstats.partial_result_cache_num_splits += 1;
                    rstats.partial_result_cache_num_docs += t.so.num_docs;
                    if (leaf_max > 0 && all_hits.size() >= leaf_max) {
                        size_t k = std::min<size_t>(leaf_max, all_hits.size());
                        std::partial_sort(all_hits.begin(), all_hits.begin() + k,
                                          all_hits.end(), cmp);
                        all_hits.resize(k);
                        if (all_hits.size() == leaf_max)
                            filter.record_new_worst_hit(all_hits.back());
                    }
                    continue;
                }
            }
            SplitResult r;
            try {
                r = search_device_split(ctx, *t.ds, t.req, schema);
            } catch (const std::exception& e) {
                // per-split failure is data, not an exception (leaf.rs:2143)
                pb::SplitSearchError se;
                se.error = e.what();
                se.split_id = t.so.split_id;
                se.retryable_error = true;
                resp.failed_splits.push_back(std::move(se));
                continue;
            }
            resp.num_successful_splits++;
            resp.num_hits += r.num_hits;
            if (cacheable) {  // cache fill on success (leaf.rs:966)
                pb::LeafSearchResponse cv;
                cv.num_hits = r.num_hits;
                cv.partial_hits = r.hits;
                if (r.has_aggs) cv.intermediate_aggregation_result = r.aggs.encode();
                ctx->leaf_cache.put(ckey, cv.encode());
            }
            for (auto& h : r.hits) all_hits.push_back(std::move(h));
            if (r.has_aggs) {
                if (!any_aggs) {
                    merged_aggs = std::move(r.aggs);
                    any_aggs = true;
                } else merged_aggs.merge(r.aggs);
            }
            // incremental top-K + worst-hit feedback (leaf.rs:2310-2317)
            if (leaf_max > 0 && all_hits.size() >= leaf_max) {
                size_t k = std::min<size_t>(leaf_max, all_hits.size());
                std::partial_sort(all_hits.begin(), all_hits.begin() + k,
                                  all_hits.end(), cmp);
                all_hits.resize(k);
                if (all_hits.size() == leaf_max)
                    filter.record_new_worst_hit(all_hits.back());
            }
            pb::SplitResourceStats ss;
            ss.split_num_docs = t.ds->total_docs;
            ss.matched_num_docs = r.num_hits;
            ss.cpu_search_microsecs = r.micros;  // GPU wall (cpu_search analog)
            rstats.localexec_num_splits++;
            rstats.localexec_num_docs += ss.split_num_docs;
            rstats.split_resources_sum.split_num_docs += ss.split_num_docs;
            rstats.split_resources_sum.matched_num_docs += ss.matched_num_docs;
            rstats.split_resources_sum.cpu_search_microsecs += ss.cpu_search_microsecs;
            if (ss.cpu_search_microsecs >= worst) {
                worst = ss.cpu_search_microsecs;
                rstats.split_resources_worst = ss;
            }
        }
        size_t k = std::min<size_t>(leaf_max, all_hits.size());
        std::partial_sort(all_hits.begin(), all_hits.begin() + k, all_hits.end(), cmp);
        all_hits.resize(k);
        resp.partial_hits = std::move(all_hits);
        if (any_aggs) resp.intermediate_aggregation_result = merged_aggs.encode();
        resp.resource_stats = rstats;
        fill_buf(out, resp.encode());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        std::string msg = e.what();
        if (msg.find("not supported") != std::string::npos ||
            msg.find("not flattenable") != std::string::npos ||
            msg.find("invalid regex") != std::string::npos ||
            msg.find("regex on unknown field") != std::string::npos ||
            msg.find("regex query on a non-text field") != std::string::npos)
            return QW_ERR_INVALID_QUERY;
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_fetch_docs(qw_ctx* ctx, const uint8_t* req_pb, size_t req_len,
                      qw_buf* out) {
    using namespace qw;
    try {
        pb::FetchDocsRequest freq = pb::FetchDocsRequest::decode(req_pb, req_len);
        // group hits by split (fetch_docs.rs:56-60 sorts GlobalDocAddress);
        // one block decompression serves consecutive docs of the same block
        std::vector<size_t> order(freq.partial_hits.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
            const pb::PartialHit& ha = freq.partial_hits[a];
            const pb::PartialHit& hb = freq.partial_hits[b];
            if (ha.split_id != hb.split_id) return ha.split_id < hb.split_id;
            if (ha.segment_ord != hb.segment_ord)
                return ha.segment_ord < hb.segment_ord;
            return ha.doc_id < hb.doc_id;
        });
        pb::FetchDocsResponse resp;
        std::string cur_split;
        uint32_t cur_seg = ~0u;
        const DeviceSplit* ds = nullptr;
        const SplitView* svp = nullptr;
        std::vector<uint8_t> block;       // decompressed block cache
        int64_t cached_block = -1;
        for (size_t oi : order) {
            const pb::PartialHit& h = freq.partial_hits[oi];
            if (h.split_id != cur_split || h.segment_ord != cur_seg) {
                auto it = ctx->splits.find(h.split_id);
                if (it == ctx->splits.end())
                    throw std::runtime_error("unknown split: " + h.split_id);
                ds = it->second.get();
                cur_split = h.split_id;
                cur_seg = h.segment_ord;
                if (ds->segs.empty()) {
                    if (h.segment_ord != 0)
                        throw std::runtime_error("bad segment ord");
                    svp = &ds->view;
                } else {
                    if (h.segment_ord >= ds->segs.size())
                        throw std::runtime_error("bad segment ord");
                    svp = &ds->segs[h.segment_ord]->view;
                }
                cached_block = -1;
            }
            const DocStoreView& d = svp->docstore;
            if (!d.present)
                throw std::runtime_error("split has no docstore: " + h.split_id);
            if (h.doc_id >= svp->num_docs)
                throw std::runtime_error("doc id out of range");
            // binary search the block whose [first, next_first) covers doc
            uint32_t lo = 0, hi = d.n_blocks;
            while (lo + 1 < hi) {
                uint32_t mid = (lo + hi) / 2;
                if (d.firsts[mid] <= h.doc_id) lo = mid;
                else hi = mid;
            }
            if (int64_t(lo) != cached_block) {
                uint32_t nb = d.firsts[lo + 1] - d.firsts[lo];
                // uncompressed size upper bound: grow until inflate fits
                uLongf dst_len = uLongf(
                    std::max<uint64_t>(64 * 1024, (d.offs[lo + 1] - d.offs[lo]) * 8));
                for (;;) {
                    block.resize(dst_len);
                    uLongf got = dst_len;
                    int rc = uncompress(block.data(), &got, d.blocks + d.offs[lo],
                                        uLong(d.offs[lo + 1] - d.offs[lo]));
                    if (rc == Z_OK) {
                        block.resize(got);
                        break;
                    }
                    if (rc != Z_BUF_ERROR)
                        throw std::runtime_error("docstore block inflate failed");
                    dst_len *= 2;
                }
                if (block.size() < nb * 4)
                    throw std::runtime_error("docstore block too short");
                cached_block = int64_t(lo);
            }
            uint32_t nb = d.firsts[lo + 1] - d.firsts[lo];
            const uint32_t* lens = (const uint32_t*)block.data();
            uint32_t local = h.doc_id - d.firsts[lo];
            uint64_t off = nb * 4ull;
            for (uint32_t i = 0; i < local; ++i) off += lens[i];
            if (off + lens[local] > block.size())
                throw std::runtime_error("docstore block corrupt");
            pb::LeafHit lh;
            lh.leaf_json.assign((const char*)block.data() + off, lens[local]);
            lh.partial_hit = h;
            resp.hits.push_back(std::move(lh));
        }
        fill_buf(out, resp.encode());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_leaf_list_terms(qw_ctx* ctx, const uint8_t* req_pb, size_t req_len,
                           qw_buf* out) {
    using namespace qw;
    try {
        pb::LeafListTermsRequest lreq = pb::LeafListTermsRequest::decode(req_pb, req_len);
        const pb::ListTermsRequest& req = lreq.list_terms_request;
        pb::LeafListTermsResponse resp;
        // per split: sorted dict range scan, limited (list_terms.rs:246-290)
        std::vector<std::vector<std::string>> per_split;
        for (auto& so : lreq.split_offsets) {
            auto it = ctx->splits.find(so.split_id);
            if (it == ctx->splits.end()) {
                pb::SplitSearchError se;
                se.split_id = so.split_id;
                se.error = "unknown split: " + so.split_id;
                se.retryable_error = true;
                resp.failed_splits.push_back(std::move(se));
                continue;
            }
            const DeviceSplit* dsp = it->second.get();
            std::vector<const SplitView*> views;
            if (dsp->segs.empty()) views.push_back(&dsp->view);
            else
                for (auto& sg : dsp->segs) views.push_back(&sg->view);
            const TextFieldView* f0 = views[0]->text_field(req.field);
            if (!f0) {
                pb::SplitSearchError se;
                se.split_id = so.split_id;
                se.error = "couldn't get field named \"" + req.field +
                           "\" from schema to list terms";
                se.retryable_error = false;
                resp.failed_splits.push_back(std::move(se));
                continue;
            }
            resp.num_attempted_splits++;
            // each segment dict is sorted: one run per segment, k-merged +
            // deduped below with the other splits' runs
            for (const SplitView* svv : views) {
                const TextFieldView* f = svv->text_field(req.field);
                if (!f) continue;
                std::vector<std::string> terms;
                for (uint32_t t = 0; t < f->num_terms; ++t) {
                    const char* s = (const char*)f->h_term_bytes + f->h_term_offsets[t];
                    size_t sl = f->h_term_offsets[t + 1] - f->h_term_offsets[t];
                    std::string term(s, sl);
                    if (req.start_key && term < *req.start_key) continue;  // ge
                    if (req.end_key && term >= *req.end_key) break;        // lt
                    terms.push_back(std::move(term));
                    if (req.max_hits && terms.size() >= *req.max_hits) break;
                }
                per_split.push_back(std::move(terms));
            }
        }
        // k-merge + dedup + global limit (list_terms.rs:291-300,392-400)
        std::vector<size_t> pos(per_split.size(), 0);
        while (true) {
            if (req.max_hits && resp.terms.size() >= *req.max_hits) break;
            const std::string* best = nullptr;
            for (size_t i = 0; i < per_split.size(); ++i)
                if (pos[i] < per_split[i].size() &&
                    (!best || per_split[i][pos[i]] < *best))
                    best = &per_split[i][pos[i]];
            if (!best) break;
            std::string v = *best;
            for (size_t i = 0; i < per_split.size(); ++i)
                while (pos[i] < per_split[i].size() && per_split[i][pos[i]] == v)
                    ++pos[i];
            resp.terms.push_back(std::move(v));
        }
        resp.num_hits = resp.terms.size();
        fill_buf(out, resp.encode());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_INTERNAL;
    }
}

void qw_buf_free(qw_buf* buf) {
    if (!buf) return;
    free(buf->data);
    buf->data = nullptr;
    buf->len = 0;
}

int32_t qw_merge_leaf_responses(const uint8_t* search_request_pb,
                                size_t search_request_len, const uint8_t** response_pbs,
                                const size_t* response_lens, size_t n,
                                qw_buf* merged_out) {
    using namespace qw;
    try {
        pb::SearchRequest req = pb::SearchRequest::decode(
            pb::Reader(search_request_pb, search_request_len));
        pb::LeafSearchResponse m;
        IntermediateAggResults aggs;
        bool any_aggs = false;
        std::vector<pb::PartialHit> all_hits;
        for (size_t i = 0; i < n; ++i) {
            pb::LeafSearchResponse r =
                pb::LeafSearchResponse::decode(response_pbs[i], response_lens[i]);
            m.num_hits += r.num_hits;
            m.num_attempted_splits += r.num_attempted_splits;
            m.num_successful_splits += r.num_successful_splits;
            for (auto& h : r.partial_hits) all_hits.push_back(std::move(h));
            for (auto& f : r.failed_splits) m.failed_splits.push_back(std::move(f));
            if (r.intermediate_aggregation_result) {
                IntermediateAggResults ir = IntermediateAggResults::decode(
                    (const uint8_t*)r.intermediate_aggregation_result->data(),
                    r.intermediate_aggregation_result->size());
                if (!any_aggs) {
                    aggs = std::move(ir);
                    any_aggs = true;
                } else aggs.merge(ir);
            }
            if (r.resource_stats) {
                if (!m.resource_stats) m.resource_stats = pb::LeafResourceStats{};
                m.resource_stats->partial_result_cache_num_splits +=
                    r.resource_stats->partial_result_cache_num_splits;
                m.resource_stats->partial_result_cache_num_docs +=
                    r.resource_stats->partial_result_cache_num_docs;
                m.resource_stats->localexec_num_splits +=
                    r.resource_stats->localexec_num_splits;
                m.resource_stats->localexec_num_docs +=
                    r.resource_stats->localexec_num_docs;
                m.resource_stats->split_resources_sum.cpu_search_microsecs +=
                    r.resource_stats->split_resources_sum.cpu_search_microsecs;
                m.resource_stats->split_resources_sum.split_num_docs +=
                    r.resource_stats->split_resources_sum.split_num_docs;
                m.resource_stats->split_resources_sum.matched_num_docs +=
                    r.resource_stats->split_resources_sum.matched_num_docs;
            }
        }
        int order1 = req.sort_fields.empty() ? 1 : req.sort_fields[0].sort_order;
        int order2 = req.sort_fields.size() > 1 ? req.sort_fields[1].sort_order : 1;
        auto cmp = [&](const pb::PartialHit& a, const pb::PartialHit& b) {
            return hit_before(a, b, order1, order2);
        };
        size_t k = std::min<size_t>(req.max_hits + req.start_offset, all_hits.size());
        std::partial_sort(all_hits.begin(), all_hits.begin() + k, all_hits.end(), cmp);
        all_hits.resize(k);
        m.partial_hits = std::move(all_hits);
        if (any_aggs) m.intermediate_aggregation_result = aggs.encode();
        fill_buf(merged_out, m.encode());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_merge_intermediate_aggs(const uint8_t** blobs, const size_t* lens,
                                   size_t n, qw_buf* merged_out) {
    using namespace qw;
    try {
        IntermediateAggResults aggs;
        for (size_t i = 0; i < n; ++i) {
            IntermediateAggResults ir =
                IntermediateAggResults::decode(blobs[i], lens[i]);
            if (i == 0) aggs = std::move(ir);
            else aggs.merge(ir);
        }
        fill_buf(merged_out, aggs.encode());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_finalize_agg_to_json(const uint8_t* blob, size_t len,
                                const char* agg_request_json, qw_buf* json_out) {
    using namespace qw;
    try {
        IntermediateAggResults ir = IntermediateAggResults::decode(blob, len);
        std::vector<AggDef> defs = parse_agg_request(agg_request_json);
        fill_buf(json_out, finalize_aggs_json(ir, defs));
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_regex_match_terms(const char* regex, size_t regex_len,
                             const uint8_t* term_bytes,
                             const uint32_t* term_offsets, size_t num_terms,
                             uint64_t* match_bitmap_out) {
    using namespace qw;
    try {
        if (!regex || !term_offsets || !match_bitmap_out ||
            (num_terms && !term_bytes && term_offsets[num_terms])) {
            set_err(nullptr, "qw_regex_match_terms: null argument");
            return QW_ERR_INVALID_ARGUMENT;
        }
        std::shared_ptr<const rx::Dfa> cached =
            rx::compile_cached(std::string(regex, regex_len));
        const rx::Dfa& dfa = *cached;
        for (size_t w = 0; w < (num_terms + 63) / 64; ++w) {
            uint64_t bits = 0;
            for (size_t t = w * 64; t < std::min(num_terms, w * 64 + 64); ++t)
                if (rx::match(dfa, term_bytes + term_offsets[t],
                              term_offsets[t + 1] - term_offsets[t]))
                    bits |= 1ull << (t & 63);
            match_bitmap_out[w] = bits;
        }
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INVALID_QUERY;
    }
}

int32_t qw_regex_table_stats(const char* regex, size_t regex_len,
                             uint64_t out[3]) {
    try {
        if (!regex || !out) {
            set_err(nullptr, "qw_regex_table_stats: null argument");
            return QW_ERR_INVALID_ARGUMENT;
        }
        std::shared_ptr<const qw::rx::Dfa> dfa =
            qw::rx::compile_cached(std::string(regex, regex_len));
        out[0] = dfa->n_states;
        out[1] = dfa->n_classes;
        out[2] = dfa->table_bytes();
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INVALID_QUERY;
    }
}

int32_t qw_regex_resolve(const char* regex, size_t regex_len,
                         int32_t tokenizer_lowercases, qw_buf* resolved_out) {
    try {
        if (!regex || !resolved_out) {
            set_err(nullptr, "qw_regex_resolve: null argument");
            return QW_ERR_INVALID_ARGUMENT;
        }
        fill_buf(resolved_out, qw::rx::resolve(std::string(regex, regex_len),
                                               tokenizer_lowercases != 0));
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(nullptr, e.what());
        return QW_ERR_INTERNAL;
    }
}

int32_t qw_kernel_stats(qw_ctx* ctx, const char* kernel_name, double* total_ms,
                        uint64_t* launches) {
    auto it = ctx->timers.find(kernel_name);
    if (it == ctx->timers.end()) {
        static const char* known[] = {"union_bm25", "range_filter", "column_agg",
                                      "topk_select", "k_dict_dfa_match",
                                      "k_terms_union_bitmap"};
        bool ok = false;
        for (const char* k : known) ok |= kernel_name == std::string(k);
        if (!ok) return QW_ERR_NOT_FOUND;
        *total_ms = 0;
        *launches = 0;
        return QW_OK;
    }
    *total_ms = it->second.total_ms;
    *launches = it->second.launches;
    return QW_OK;
}

void qw_kernel_stats_reset(qw_ctx* ctx) { ctx->timers.clear(); }

int32_t qw_ctx_memory_stats(qw_ctx* ctx, uint64_t* used_bytes,
                            uint64_t* budget_bytes, uint64_t* splits_bytes) {
    if (!ctx) return QW_ERR_INVALID_ARGUMENT;
    if (used_bytes) *used_bytes = ctx->hbm_used + ctx->hitsets.bytes;
    if (budget_bytes) *budget_bytes = ctx->hbm_budget;
    if (splits_bytes) {
        uint64_t sb = 0;
        for (auto& kv : ctx->splits) sb += kv.second->len + 64;
        *splits_bytes = sb;
    }
    return QW_OK;
}

int32_t qw_absence_cache_stats(qw_ctx* ctx, uint64_t* hits, uint64_t* misses,
                               uint64_t* entries) {
    if (!ctx) return QW_ERR_INVALID_ARGUMENT;
    if (hits) *hits = ctx->absence.hits;
    if (misses) *misses = ctx->absence.misses;
    if (entries) *entries = uint64_t(ctx->absence.keys.size());
    return QW_OK;
}

int32_t qw_topk_stats(qw_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return QW_ERR_INVALID_ARGUMENT;
    out[0] = ctx->topk_pruned;
    out[1] = ctx->topk_unpruned;
    out[2] = ctx->topk_last_emitted;
    out[3] = ctx->topk_last_matched;
    return QW_OK;
}

int32_t qw_topk_onesync_stats(qw_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return QW_ERR_INVALID_ARGUMENT;
    out[0] = ctx->topk_onesync_calls;
    out[1] = ctx->topk_onesync_fallbacks;
    out[2] = ctx->topk_onesync_last_survivors;
    out[3] = ctx->topk_onesync_last_tail;
    return QW_OK;
}

int32_t qw_ctx_device_sync(qw_ctx* ctx) {
    try {
        ctx_ensure_device(ctx);
        HIP_CHECK(hipDeviceSynchronize());
        return QW_OK;
    } catch (const std::exception& e) {
        set_err(ctx, e.what());
        return QW_ERR_NO_GPU;
    }
}

}  // extern "C"
