"""terms -> percentiles on the device: the tile kernel's pass
over every ordinal, the per-split cut to the kept terms, and the second pass
(k_terms_perc_sketch) that sketches the kept buckets. Every case is compared
with the pure-Python reference over the documents, rendered doubles for
equality.
"""
import json
import os

import pytest
import torch.multiprocessing as mp

import terms_percentiles_corpora as corp
import terms_percentiles_reference as ref
from quickwit_amd import proto, splitgen
from quickwit_amd.api import make_leaf_request

pytestmark = pytest.mark.gpu

PERCENTS = [1, 25, 50, 75, 95, 99.9]


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def corpora():
    return corp.small_corpora()


@pytest.fixture(scope="module")
def bulk():
    ords, grp, lat = corp.bulk_corpus()
    return corp.bulk_docs(ords, grp, lat), corp.bulk_split(ords, grp, lat, "bulk")


@pytest.fixture(scope="module")
def gpu(corpora, bulk):
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)
    for name, docs in corpora.items():
        g.add_split(name, corp.write_split(docs, name))
    g.add_split("bulk", bulk[1])
    segs = corp.segment_docs()
    g.add_split("seg3", splitgen.concat_segments(
        [corp.write_split(d, "seg3") for d in segs], "seg3"))
    return g


def search(gpu, sid, ndocs, query, aggs, schema=corp.SCHEMA, max_hits=0, **kw):
    return gpu.leaf_search(make_leaf_request(
        query, schema, [(sid, ndocs)], max_hits=max_hits, aggregation=aggs,
        **kw))


def agg_json(gpu, resp, aggs):
    assert not resp.get("failed_splits"), resp.get("failed_splits")
    return gpu.finalize_agg_json(resp["intermediate_aggregation_result"], aggs)


def terms_aggs(field="svc", sub="lat", size=10, **terms_kw):
    return {"t": {"terms": dict(field=field, size=size, **terms_kw), "aggs": {
        "p": {"percentiles": {"field": sub, "percents": PERCENTS}}}}}


def want_buckets(docs, field, sub, size, match=None):
    groups = ref.terms_percentiles(docs, field, sub, PERCENTS, match)
    return [(t, g["doc_count"], g["values"])
            for t, g in ref.shown_buckets(groups, size)]


def got_buckets(j):
    return [(b["key"], b["doc_count"], b["p"]["values"])
            for b in j["t"]["buckets"]]


def check(gpu, sid, docs, query=corp.Q_ALL, match=None, field="svc",
          sub="lat", size=10, schema=corp.SCHEMA, **terms_kw):
    aggs = terms_aggs(field, sub, size, **terms_kw)
    j = agg_json(gpu, search(gpu, sid, len(docs), query, aggs, schema), aggs)
    want = want_buckets(docs, field, sub, size, match)
    assert got_buckets(j) == want
    return j, want


# ---- (a) tile edges
def test_one_document(gpu, corpora):
    _j, want = check(gpu, "one_doc", corpora["one_doc"])
    assert len(want) == 1 and want[0][1] == 1


def test_one_tile_plus_37_documents(gpu, corpora):
    docs = corpora["tile_plus_37"]
    assert len(docs) == corp.TILE_DOCS + 37
    check(gpu, "tile_plus_37", docs)
    # a term query matching a strict subset; the last 37 docs are in it
    _j, want = check(gpu, "tile_plus_37", docs, corp.Q_SUBSET, corp.in_subset)
    assert 0 < sum(w[1] for w in want) < len(docs)
    assert any(corp.in_subset(d) for d in docs[corp.TILE_DOCS:])


def test_query_matching_nothing(gpu, corpora):
    docs = corpora["tile_plus_37"]
    aggs = terms_aggs()
    resp = search(gpu, "tile_plus_37", len(docs), corp.Q_NONE, aggs)
    assert resp.get("num_hits", 0) == 0
    assert agg_json(gpu, resp, aggs)["t"]["buckets"] == []


# ---- (b) ordinal widths 1, 2, 4
def test_ordinal_width_1_none_dropped(gpu, corpora):
    # 5 terms, split_size 25: every ordinal is kept
    _j, want = check(gpu, "width1", corpora["width1"], corp.Q_SUBSET,
                     corp.in_subset)
    assert len(want) == 5


def test_ordinal_width_2(gpu, corpora):
    docs = corpora["width2"]
    assert 256 < len({d["svc"] for d in docs}) <= 300
    check(gpu, "width2", docs, size=10)           # 25 of ~300 kept
    check(gpu, "width2", docs, corp.Q_SUBSET, corp.in_subset, size=10)
    check(gpu, "width2", docs, size=300, split_size=400)  # none dropped


def test_ordinal_width_4_most_dropped(gpu, bulk):
    docs = bulk[0]
    assert len(docs) == corp.BULK_DOCS
    assert len({d["svc"] for d in docs}) == corp.BULK_CARD
    check(gpu, "bulk", docs, size=3, schema=corp.BULK_SCHEMA)  # 14 kept
    check(gpu, "bulk", docs, corp.Q_SUBSET, corp.in_subset, size=3,
          schema=corp.BULK_SCHEMA)


# ---- (c) the match set is the one pass 1 counted over
def test_bucket_equals_top_level_percentiles_under_term_filter(gpu, corpora):
    from test_terms_percentiles_cpu import decode_terms_blob
    docs = corpora["width1"]  # lat has no nulls
    assert all("lat" in d for d in docs)
    aggs = terms_aggs()
    resp = search(gpu, "width1", len(docs), corp.Q_SUBSET, aggs)
    j = agg_json(gpu, resp, aggs)
    top = {"p": {"percentiles": {"field": "lat", "percents": PERCENTS}}}
    assert len(j["t"]["buckets"]) == 5
    for b in j["t"]["buckets"]:
        q = {"type": "bool", "must": [
            corp.Q_SUBSET, {"type": "term", "field": "svc", "value": b["key"]}]}
        r = search(gpu, "width1", len(docs), q, top)
        assert r["num_hits"] == b["doc_count"]
        assert agg_json(gpu, r, top)["p"]["values"] == b["p"]["values"]
    _n, _s, entries, _m, _e = decode_terms_blob(
        resp["intermediate_aggregation_result"])
    for key, dc, (sk,) in entries:
        assert sk[1] + sum(sk[2].values()) == dc, key


# ---- (d) nulls
def test_nullable_sub_column_and_all_null_bucket(gpu, corpora):
    docs = corpora["all_null_bucket"]
    j, _want = check(gpu, "all_null_bucket", docs)
    nul = [b for b in j["t"]["buckets"] if b["key"] == "nul"][0]
    assert nul["doc_count"] > 0
    assert nul["p"]["values"] == {ref.percent_key(p): None for p in PERCENTS}


def test_nullable_terms_column(gpu, corpora):
    docs = corpora["nullable"]
    assert any("svc" not in d for d in docs)
    check(gpu, "nullable", docs)
    check(gpu, "nullable", docs, corp.Q_SUBSET, corp.in_subset)


# ---- (e) multi-valued terms column
def test_multi_valued_terms_column(gpu, corpora):
    docs = corpora["nullable"]
    assert any(len(d["tags"]) > 1 for d in docs)
    assert any(len(d["tags"]) == 0 for d in docs)
    check(gpu, "nullable", docs, field="tags")
    check(gpu, "nullable", docs, corp.Q_SUBSET, corp.in_subset, field="tags")


# ---- (f) u64 / i64 / f64 sub columns, the zero bucket, a deep table
@pytest.mark.parametrize("sub", ["lat", "cnt", "dl"])
def test_value_types_and_zero_bucket(gpu, corpora, sub):
    docs = corpora["zeroes"]
    assert any(d.get(sub) == 0 for d in docs)
    j, _want = check(gpu, "zeroes", docs, sub=sub)
    assert any(b["p"]["values"]["1.0"] == 0.0 for b in j["t"]["buckets"])


def test_values_spanning_twelve_decades(gpu, corpora):
    docs = corpora["wide"]
    lats = [d["lat"] for d in docs]
    assert min(lats) < 2e-3 and max(lats) > 5e8
    check(gpu, "wide", docs)
    check(gpu, "wide", docs, corp.Q_SUBSET, corp.in_subset)


def test_boundary_table_too_large_for_lds(gpu, corpora):
    """the two kernel paths that search the table in global memory: with
    global counters (5 rows x 17,600 keys) and with LDS counters (1 row)"""
    lats = [d["lat"] for d in corpora["huge"]]
    assert min(lats) < 1e-2 and max(lats) > 1e148
    check(gpu, "huge", corpora["huge"], corp.Q_SUBSET, corp.in_subset)
    lats = [d["lat"] for d in corpora["one_term"]]
    assert max(lats) > 1e39 and len({d["svc"] for d in corpora["one_term"]}) == 1
    check(gpu, "one_term", corpora["one_term"])


# ---- (g) several subs and orders
def test_two_percentiles_subs_a_stats_sub_and_orders(gpu, corpora):
    docs = corpora["width1"]
    groups = ref.terms_percentiles(docs, "svc", "lat", PERCENTS)
    groups2 = ref.terms_percentiles(docs, "svc", "cnt", [50])
    avg = {}
    for t in groups:
        v = [d["dl"] for d in docs if d.get("svc") == t]
        avg[t] = sum(v) / len(v)
    for order, key in (
            ({"st.avg": "desc"}, lambda kv: (-avg[kv[0]], kv[0])),
            ({"_count": "asc"}, lambda kv: (kv[1]["doc_count"], kv[0]))):
        aggs = {"t": {"terms": {"field": "svc", "size": 3, "order": order},
                      "aggs": {
            "p": {"percentiles": {"field": "lat", "percents": PERCENTS}},
            "st": {"stats": {"field": "dl"}},
            "p2": {"percentiles": {"field": "cnt", "percents": [50],
                                   "keyed": False}}}}}
        j = agg_json(gpu, search(gpu, "width1", len(docs), corp.Q_ALL, aggs),
                     aggs)
        want = ref.shown_buckets(groups, 3, key)
        assert [(b["key"], b["doc_count"], b["p"]["values"])
                for b in j["t"]["buckets"]] == [
            (t, g["doc_count"], g["values"]) for t, g in want]
        for b in j["t"]["buckets"]:
            assert b["p2"]["values"] == [
                {"key": 50.0, "value": groups2[b["key"]]["values"]["50.0"]}]
            assert b["st"]["count"] == b["doc_count"]
            assert b["st"]["avg"] == pytest.approx(avg[b["key"]], rel=1e-12)


# ---- (h) QWA2: three segments, three dictionaries
def test_three_segments_with_different_dictionaries(gpu):
    segs = corp.segment_docs()
    dicts = [{d["svc"] for d in s if "svc" in d} for s in segs]
    assert dicts[0] != dicts[1] != dicts[2] and dicts[0] & dicts[1] & dicts[2]
    docs = [d for s in segs for d in s]
    _j, want = check(gpu, "seg3", docs, size=20)
    assert {"only0", "only1", "only2"} <= {w[0] for w in want}
    check(gpu, "seg3", docs, corp.Q_SUBSET, corp.in_subset, size=20)


# ---- (i) hits, search_after and the hitset cache leave the result alone
def test_hits_search_after_and_cache_do_not_change_the_aggregation(corpora):
    from quickwit_amd.api import GpuSearcher
    docs = corpora["nullable"]
    g = GpuSearcher(device=0)  # fresh: the first request finds the cache cold
    g.add_split("nullable", corp.write_split(docs, "nullable"))
    aggs = terms_aggs()
    want = want_buckets(docs, "svc", "lat", 10, corp.in_subset)
    cold = agg_json(g, search(g, "nullable", len(docs), corp.Q_SUBSET, aggs),
                    aggs)
    warm = agg_json(g, search(g, "nullable", len(docs), corp.Q_SUBSET, aggs),
                    aggs)
    assert got_buckets(cold) == want
    assert warm == cold
    sort = [{"field_name": "ts", "sort_order": 1}]
    page = search(g, "nullable", len(docs), corp.Q_SUBSET, aggs, max_hits=5,
                  sort_fields=sort)
    assert len(page["partial_hits"]) == 5
    assert agg_json(g, page, aggs) == cold
    req = make_leaf_request(corp.Q_SUBSET, corp.SCHEMA,
                            [("nullable", len(docs))], max_hits=5,
                            sort_fields=sort, aggregation=aggs)
    req["search_request"]["search_after"] = page["partial_hits"][-1]
    after = g.leaf_search(req)
    assert after["partial_hits"] and (
        after["partial_hits"][0] != page["partial_hits"][0])
    assert agg_json(g, after, aggs) == cold


# ---- (j) refusals arrive as failed splits and leak no HBM
def _refusal(g, sid, ndocs, schema, aggs, warm_aggs, message):
    # the same request with a stats sub in the percentiles sub's place grows
    # the context's scratch buffers to their final size first
    assert not search(g, sid, ndocs, corp.Q_ALL, warm_aggs, schema).get(
        "failed_splits")
    used = g.memory_stats()[0]
    resp = search(g, sid, ndocs, corp.Q_ALL, aggs, schema)
    failed = resp.get("failed_splits", [])
    assert len(failed) == 1 and failed[0]["split_id"] == sid
    assert message in failed[0]["error"], failed[0]["error"]
    assert g.memory_stats()[0] == used


def _with_stats_sub(aggs, field):
    warm = json.loads(json.dumps(aggs))
    warm["t"]["aggs"]["p"] = {"avg": {"field": field}}
    warm["t"]["terms"].pop("order", None)
    return warm


def test_refusals(gpu, corpora, bulk):
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)
    docs = [dict(d, dl=d["dl"] - 3000) for d in corpora["width1"]]
    assert min(d["dl"] for d in docs) < 0
    g.add_split("neg", corp.write_split(docs, "neg"))
    g.add_split("bulk", bulk[1])
    n = len(docs)
    aggs = terms_aggs(sub="dl")
    _refusal(g, "neg", n, corp.SCHEMA, aggs, _with_stats_sub(aggs, "dl"),
             "percentiles over negative values")
    aggs = terms_aggs(order={"p.95": "desc"})
    _refusal(g, "neg", n, corp.SCHEMA, aggs, _with_stats_sub(aggs, "lat"),
             "unknown stat")
    # 66,000 kept rows x about 1,400 keys is past 2^25 words
    aggs = terms_aggs(size=3, split_size=100_000)
    _refusal(g, "bulk", corp.BULK_DOCS, corp.BULK_SCHEMA, aggs,
             _with_stats_sub(aggs, "lat"),
             "percentiles sketch region too large")
    # numeric-keyed terms carry no sub-aggregations: refused, not nulls
    aggs = terms_aggs(field="cnt")
    _refusal(g, "neg", n, corp.SCHEMA, aggs, _with_stats_sub(aggs, "lat"),
             "percentiles under terms over a numeric column")


def test_budget_refusal_inside_pass_2_frees_its_buffers(bulk):
    """The region allocation meets the HBM budget when pass 2 already holds
    its remap table and boundary table on the device: the holder frees them
    and the split fails with the budget message."""
    import re
    from quickwit_amd.api import GpuSearcher
    small = terms_aggs(size=3)

    def warmed(config):
        # grows the scratch buffers and memoizes the match bitmap
        g = GpuSearcher(device=0, config=config)
        g.add_split("bulk", bulk[1])
        agg_json(g, search(g, "bulk", corp.BULK_DOCS, corp.Q_ALL, small,
                           corp.BULK_SCHEMA), small)
        return g

    used = warmed(None).memory_stats()[0]
    g = warmed({"hbm_memory_budget": used + (2 << 20)})
    assert g.memory_stats()[0] == used
    # 20,000 kept rows x about 1,400 keys: under 2^25 words, 220 MB of u64;
    # the remap (264 KB) and the table (11 KB) fit the 2 MiB left
    kept = 20_000
    aggs = terms_aggs(size=3, split_size=kept)
    resp = search(g, "bulk", corp.BULK_DOCS, corp.Q_ALL, aggs,
                  corp.BULK_SCHEMA)
    failed = resp.get("failed_splits", [])
    assert len(failed) == 1, resp
    assert "HBM memory budget exceeded" in failed[0]["error"]
    need = int(re.search(r"need (\d+)", failed[0]["error"]).group(1))
    assert need > (100 << 20) and need % (kept * 8) == 0  # the region
    assert g.memory_stats()[0] == used
    # and the context still answers
    assert got_buckets(agg_json(g, search(
        g, "bulk", corp.BULK_DOCS, corp.Q_ALL, small, corp.BULK_SCHEMA),
        small)) == want_buckets(bulk[0], "svc", "lat", 3)


# ---- (k) world-2 merge equals the single call
def _rank_main(rank, world, port, result):
    import torch
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from quickwit_amd.api import GpuSearcher
    from quickwit_amd.merge import distributed_merge

    sid = "segment%d" % rank
    docs = corp.segment_docs()[rank]
    s = GpuSearcher(device=0)
    s.add_split(sid, corp.write_split(docs, sid))
    req = make_leaf_request(corp.Q_SUBSET, corp.SCHEMA, [(sid, len(docs))],
                            max_hits=5, aggregation=terms_aggs(size=20))
    resp_pb = s.leaf_search_raw(proto.encode("LeafSearchRequest", req))
    sreq_pb = proto.encode("SearchRequest", req["search_request"])
    merged = distributed_merge(sreq_pb, resp_pb, [sid],
                               device=torch.device("cpu"))
    if rank == 0:
        result.put(merged)
    dist.destroy_process_group()


def test_two_rank_merge_equals_single_call(gpu, corpora):
    ctx = mp.get_context("spawn")
    result = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, 29541, result))
             for r in range(2)]
    for p in procs:
        p.start()
    merged = proto.decode("LeafSearchResponse", result.get(timeout=180))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    aggs = terms_aggs(size=20)
    splits = [("segment%d" % r, len(corpora["segment%d" % r]))
              for r in range(2)]
    single = gpu.leaf_search(make_leaf_request(
        corp.Q_SUBSET, corp.SCHEMA, splits, max_hits=5, aggregation=aggs))
    assert merged["num_hits"] == single["num_hits"]
    gj = agg_json(gpu, merged, aggs)
    assert gj == agg_json(gpu, single, aggs)
    docs = corpora["segment0"] + corpora["segment1"]
    assert got_buckets(gj) == want_buckets(docs, "svc", "lat", 20,
                                           corp.in_subset)
