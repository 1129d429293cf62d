"""Scored nested boolean queries on the device: the term leaves of a tree
that does not flatten run as should terms of the tile kernel whose BM25
contribution is gated by a bitmap (the AND of the match sets of the bools
between the leaf and the root).

GpuSearcher is compared with tests/score_tree_reference.py (float64, proven
against the oracle by test_score_tree_cpu.py) under that module's comparison
rule. The corpus has three tiles, the last partial; a dense term whose
blocks straddle both tile edges, a term with one short block, a term absent
from the middle tile and a term missing from the dictionary.

Before the gated path every case of CASES came back as a failed split.
"""
import pytest

import score_tree_reference as ref
from quickwit_amd import splitgen
from quickwit_amd.api import make_leaf_request

pytestmark = pytest.mark.gpu

TWO_SEG = "score-tree-2seg"


@pytest.fixture(scope="module")
def gpu():
    import __graft_entry__
    __graft_entry__.build()
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)
    c = ref.corpus()
    g.add_split(c.split_id, c.data)
    return g


def request(node, sort, max_hits, **kw):
    c = ref.corpus()
    return make_leaf_request(node, ref.SCHEMA, [(c.split_id, c.num_docs)],
                             max_hits=max_hits,
                             sort_fields=ref.tr.sort_fields(sort), **kw)


def search(gpu, node, sort, max_hits, **kw):
    r = gpu.leaf_search(request(node, sort, max_hits, **kw))
    assert not r.get("failed_splits"), r.get("failed_splits")
    return r


def launches(gpu, name):
    try:
        return gpu.kernel_stats(name)[1]
    except KeyError:  # no launch under that name yet
        return 0


@pytest.mark.parametrize("name,node", ref.CASES, ids=[n for n, _ in ref.CASES])
def test_case_matches_reference(gpu, name, node):
    c = ref.corpus()
    n, full = ref.ranked(c, node, ref.SCORE_DESC)
    r = search(gpu, node, ref.SCORE_DESC, c.num_docs)
    assert r.get("num_hits", 0) == n, name
    worst = ref.compare(ref.hits_of(r), full, 0, c.num_docs, name)
    print(f"{name}: {n} hits, worst relative score deviation {worst:.3g}")


def test_gate_keeps_b_score_from_docs_without_c(gpu):
    """must[a], should[bool(must[b, c])]: a doc with 'b' but not 'c' scores
    'a' alone — the ungated sum a + b is what a wrong gate would give."""
    c = ref.corpus()
    node = ref.CASES[0][1]
    got = dict(ref.hits_of(search(gpu, node, ref.SCORE_DESC, c.num_docs)))
    _, sa = ref.evaluate(c, ref.term("a"))
    _, sb = ref.evaluate(c, ref.term("b"))
    b_only = [d for d in got if c.tf("b")[d] > 0 and c.tf("c")[d] == 0]
    assert len(b_only) > 1000
    for d in b_only:
        assert abs(got[d] - sa[d]) <= ref.REL * sa[d], d
        assert sb[d] > 0.1 * sa[d]  # the wrong answer is far outside REL


def test_gated_launches_have_a_timer_of_their_own(gpu):
    """A leaf under a should-edge bool runs the gated instantiation; a tree
    whose leaves need no gate (msm 2 over plain terms) runs the plain one."""
    g0, p0 = launches(gpu, "union_bm25_gated"), launches(gpu, "union_bm25")
    search(gpu, ref.OR_OF_ANDS, ref.SCORE_DESC, 10)
    assert launches(gpu, "union_bm25_gated") == g0 + 1
    assert launches(gpu, "union_bm25") == p0
    search(gpu, dict(ref.CASES)["msm2-of-3"], ref.SCORE_DESC, 10)
    assert launches(gpu, "union_bm25_gated") == g0 + 1
    assert launches(gpu, "union_bm25") > p0


def test_combined_gate_is_freed_after_the_search(gpu):
    """The depth-3 case ANDs two node bitmaps into a temporary gate; the
    HBM accounting is back where it was once the search has ended (the
    first run leaves the memoized node bitmaps and grown scratch behind)."""
    node = dict(ref.CASES)["depth3-two-gates"]
    search(gpu, node, ref.SCORE_DESC, 10)
    used = gpu.memory_stats()[0]
    search(gpu, node, ref.SCORE_DESC, 10)
    assert gpu.memory_stats()[0] == used


# ------------------------------------------------------- downstream stages
def test_score_ascending(gpu):
    c = ref.corpus()
    n, full = ref.ranked(c, ref.OR_OF_ANDS, ref.SCORE_ASC)
    r = search(gpu, ref.OR_OF_ANDS, ref.SCORE_ASC, c.num_docs)
    assert r.get("num_hits", 0) == n
    ref.compare(ref.hits_of(r), full, 0, c.num_docs, "asc")


def test_column_then_score_uses_wide_records(gpu):
    c = ref.corpus()
    sort = [("u", ref.DESC), ("_score", ref.DESC)]
    n, full = ref.ranked(c, ref.OR_OF_ANDS, sort)
    r = search(gpu, ref.OR_OF_ANDS, sort, c.num_docs)
    assert r.get("num_hits", 0) == n
    ref.compare(ref.hits_of(r), full, 0, c.num_docs, "u-then-score")
    u = [(h.get("sort_value") or {}).get("u64")
         for h in r.get("partial_hits", [])]
    assert u == [k[0] for _, _, k in full]


def test_search_after_on_score(gpu):
    """The cursor is the third hit; it sits in the five-doc top group, whose
    two-term sums are exact, so the page after it is determined."""
    c = ref.corpus()
    _, full = ref.ranked(c, ref.OR_OF_ANDS, ref.SCORE_DESC)
    first = search(gpu, ref.OR_OF_ANDS, ref.SCORE_DESC, 3)
    h = first["partial_hits"][2]
    assert h.get("doc_id", 0) == full[2][0]
    cur = {"sort_value": h["sort_value"], "split_id": c.split_id,
           "segment_ord": 0, "doc_id": h.get("doc_id", 0)}
    req = request(ref.OR_OF_ANDS, ref.SCORE_DESC, 50)
    req["search_request"]["search_after"] = cur
    r = gpu.leaf_search(req)
    assert not r.get("failed_splits"), r.get("failed_splits")
    ref.compare(ref.hits_of(r), full, 3, 50, "search_after")


@pytest.mark.parametrize("max_hits", [5, 100])
def test_max_hits_in_and_beyond_the_pruned_range(gpu, max_hits):
    """5 runs the pruned instantiation (K <= 64), 100 the unpruned one."""
    c = ref.corpus()
    n, full = ref.ranked(c, ref.OR_OF_ANDS, ref.SCORE_DESC)
    before = gpu.topk_stats()
    r = search(gpu, ref.OR_OF_ANDS, ref.SCORE_DESC, max_hits)
    after = gpu.topk_stats()
    assert r.get("num_hits", 0) == n
    ref.compare(ref.hits_of(r), full, 0, max_hits, max_hits)
    which = 0 if max_hits <= 64 else 1  # (pruned, unpruned, emitted, matched)
    assert after[which] == before[which] + 1
    if max_hits <= 64:
        assert after[2] < after[3] == n  # pruning really dropped candidates


def test_count_only_with_terms_aggregation(gpu):
    from quickwit_amd.api import OracleSearcher
    c = ref.corpus()
    cpu = OracleSearcher()
    cpu.add_split(c.split_id, c.data)
    aggs = {"t": {"terms": {"field": "u", "size": 10}}}
    req = request(ref.OR_OF_ANDS, ref.SCORE_DESC, 0, aggregation=aggs)
    g, e = gpu.leaf_search(req), cpu.leaf_search(req)
    assert not g.get("failed_splits"), g.get("failed_splits")
    n, _ = ref.ranked(c, ref.OR_OF_ANDS, ref.SCORE_DESC)
    assert g.get("num_hits", 0) == e.get("num_hits", 0) == n
    assert not g.get("partial_hits")
    assert gpu.finalize_agg_json(g["intermediate_aggregation_result"], aggs) \
        == cpu.finalize_agg_json(e["intermediate_aggregation_result"], aggs)


def test_two_segments_match_oracle():
    """Per-segment gated launches (each segment has its own dictionary, node
    bitmaps and gates) merged within the split; compared with the oracle,
    the judge of multi-segment order. All hits are returned, so no tie
    group (hits the oracle scores alike) is cut."""
    import math
    from quickwit_amd.api import GpuSearcher, OracleSearcher
    a, b = ref.corpus(), ref.second_segment()
    data = splitgen.concat_segments([a.data, b.data], TWO_SEG)
    total = a.num_docs + b.num_docs
    gpu, cpu = GpuSearcher(device=0), OracleSearcher()
    gpu.add_split(TWO_SEG, data)
    cpu.add_split(TWO_SEG, data)
    for name in ("or-of-ands", "depth3-two-gates", "absent-middle-gated"):
        node = dict(ref.CASES)[name]
        req = make_leaf_request(
            node, ref.SCHEMA, [(TWO_SEG, total)], max_hits=total,
            sort_fields=ref.tr.sort_fields(ref.SCORE_DESC))
        g, e = gpu.leaf_search(req), cpu.leaf_search(req)
        assert not g.get("failed_splits"), g.get("failed_splits")
        assert not e.get("failed_splits"), e.get("failed_splits")
        want = sum(ref.ranked(s, node)[0] for s in (a, b))
        assert g.get("num_hits", 0) == e.get("num_hits", 0) == want
        gh, eh = g["partial_hits"], e["partial_hits"]
        assert len(gh) == len(eh) == want
        groups = ({}, {})
        for x, y in zip(gh, eh):
            gs, es = x["sort_value"]["f64"], y["sort_value"]["f64"]
            assert math.isclose(gs, es, rel_tol=ref.REL, abs_tol=0.0), name
            for grp, h in zip(groups, (x, y)):
                grp.setdefault(es, set()).add(
                    (h.get("segment_ord", 0), h.get("doc_id", 0)))
        assert groups[0] == groups[1], name


# ------------------------------------------------------- regression guards
def test_phrase_under_score_is_still_refused(gpu):
    node = ref.bool_(should=["a", {
        "type": "full_text", "field": ref.FIELD, "text": "a b",
        "params": {"mode": {"type": "phrase"}}}])
    r = gpu.leaf_search(request(node, ref.SCORE_DESC, 10))
    assert r.get("failed_splits"), r
    assert "const-score" in r["failed_splits"][0].get("error", "")


def test_flattenable_scored_query_is_unchanged(gpu):
    c = ref.corpus()
    node = ref.bool_(must=["a"], should=["b", "c"], must_not=["x"])
    g0 = launches(gpu, "union_bm25_gated")
    n, full = ref.ranked(c, node, ref.SCORE_DESC)
    r = search(gpu, node, ref.SCORE_DESC, c.num_docs)
    assert r.get("num_hits", 0) == n
    ref.compare(ref.hits_of(r), full, 0, c.num_docs, "flattenable")
    assert launches(gpu, "union_bm25_gated") == g0
