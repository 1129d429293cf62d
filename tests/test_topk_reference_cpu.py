"""Proves tests/topk_reference.py — the float64 scores, the match sets and
the ordering rule — against the oracle, before a GPU is involved.

For every corpus and query test_topk_exact.py uses: the reference's match
count equals the oracle's; its expected hit list equals the oracle's ids
exactly wherever the reference calls the order determined (at most two
scoring terms, and every unscored sort); each reference score is within the
project's 1e-5 of the oracle's. One full-length request per case covers every
max_hits the GPU file asks for, since each is a prefix of that list; the
prefix rule itself (start_offset + max_hits hits per leaf) is checked too.

It also asserts the corpora's own precondition on the reference alone: any
two distinct score classes of a query differ by at least 1e-3 relative,
100 times the tolerance, so no tolerance can blur a class edge.

Decided here for the GPU file: an f64 column orders -0.0 below 0.0 (the
monotonic bit map), and a leaf's response carries the sign of zero.
"""
import math

import pytest

import topk_reference as ref
from quickwit_amd.api import OracleSearcher, make_leaf_request

CLASS_GAP = 1e-3


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


_ORACLES = {}


def oracle_for(c):
    if c.split_id not in _ORACLES:
        s = OracleSearcher()
        s.add_split(c.split_id, c.data)
        _ORACLES[c.split_id] = s
    return _ORACLES[c.split_id]


def run(c, q, sort, max_hits, start_offset=0, after=None):
    req = make_leaf_request(q.ast(), ref.SCHEMA, [(c.split_id, c.num_docs)],
                            max_hits=max_hits, start_offset=start_offset,
                            sort_fields=ref.sort_fields(sort) or None)
    if after is not None:
        req["search_request"]["search_after"] = after
    return ref.hits_of(oracle_for(c).leaf_search(req))


DETERMINED = ref.determined_cases()


@pytest.mark.parametrize("case", DETERMINED, ids=[c[0] for c in DETERMINED])
def test_determined_case_matches_oracle(case):
    name, corpus, q, sort, ks = case
    c = corpus()
    assert ref.order_determined(q, sort)
    got = run(c, q, sort, c.num_docs)
    ref.assert_hits_exact(got, ref.expected(c, q, sort, c.num_docs), sort, name)
    k = ks[len(ks) // 2]
    got = run(c, q, sort, k)
    ref.assert_hits_exact(got, ref.expected(c, q, sort, k), sort, (name, k))


def test_leaf_returns_offset_plus_max_hits():
    c = ref.tied_corpus()
    got = run(c, ref.AA, ref.SCORE_DESC, 10, start_offset=5_000)
    exp = ref.expected(c, ref.AA, ref.SCORE_DESC, 10, start_offset=5_000)
    assert len(exp[1]) == 5_010
    ref.assert_hits_exact(got, exp, ref.SCORE_DESC)


@pytest.mark.parametrize("name,q", ref.ORDER_DEPENDENT,
                         ids=[n for n, _ in ref.ORDER_DEPENDENT])
def test_order_dependent_case_scores_and_count(name, q):
    """Three and five scoring terms: the order inside a score class is the
    engine's own (f32 sum order), so only count and scores are compared."""
    c = ref.classes_corpus()
    assert not ref.order_determined(q, ref.SCORE_DESC)
    n, hits = run(c, q, ref.SCORE_DESC, c.num_docs)
    n_ref, exp = ref.ranked(c, q, ref.SCORE_DESC)
    assert n == n_ref == len(hits)
    want = {d: s for d, s, _ in exp}
    assert {h[0] for h in hits} == set(want)
    for d, s, _ in hits:
        assert abs(s - want[d]) <= ref.REL * want[d], (d, s, want[d])


@pytest.mark.parametrize("case", ref.AFTER_CASES,
                         ids=[c[0] for c in ref.AFTER_CASES])
def test_search_after_pages_match_oracle(case):
    name, corpus, q, sort = case
    c = corpus()
    n, full = ref.ranked(c, q, sort)
    field = sort[0][0]
    # every doc of the tied corpus has one score: the engine's own value of
    # it, for score cursors, comes from a one-hit response
    score = run(c, q, sort, 1)[1][0][1] if field == "_score" else None
    for r in ref.AFTER_RANKS:
        cur = ref.cursor_of(c, full[r], field, score=score)
        got = run(c, q, sort, ref.AFTER_PAGE, after=cur)
        ref.assert_hits_exact(
            got, (n, full[r + 1:r + 1 + ref.AFTER_PAGE]), sort, (name, r))
        # value-only cursor: the whole tie group of the cursor is skipped
        cur = ref.cursor_of(c, full[r], field, with_doc=False, score=score)
        rest = [h for h in full[r + 1:] if h[1] != full[r][1]]
        got = run(c, q, sort, ref.AFTER_PAGE, after=cur)
        ref.assert_hits_exact(got, (n, rest[:ref.AFTER_PAGE]), sort,
                              (name, r, "value-only"))


@pytest.mark.parametrize("n", ref.EDGE_SIZES)
def test_edge_sweep_matches_oracle(n):
    c = ref.edge_corpus(n)
    for name, q, sort, k in ref.edge_queries(n):
        assert ref.order_determined(q, sort)
        ref.assert_hits_exact(run(c, q, sort, k), ref.expected(c, q, sort, k),
                              sort, (n, name))


def test_score_classes_are_separated():
    """Precondition of every scored case, on the reference alone."""
    c = ref.classes_corpus()
    for q in (ref.AA, ref.BB_CC, ref.Q3, ref.Q5):
        gap = ref.min_class_gap(c, q)
        assert gap >= CLASS_GAP, (q.key(), gap)
    # docs of one class share one float64 score: the class sizes come out
    _, counts = ref.score_classes(c, ref.AA)
    assert counts == [3, 17_000, 100, 30_000, 22_897]
    assert len(ref.score_classes(ref.tied_corpus(), ref.AA)[0]) == 1
    for n in ref.EDGE_SIZES:
        for _, q, sort, _ in ref.edge_queries(n):
            if q.scoring_terms and sort and sort[0][0] == "_score":
                assert ref.min_class_gap(ref.edge_corpus(n), q) >= CLASS_GAP


def test_negative_zero_sorts_below_zero():
    """What the f64 sort must do with the two zeros, decided on the oracle:
    ascending, every -0.0 doc comes before every 0.0 doc, and the response
    keeps the sign."""
    c = ref.tied_corpus()
    _, hits = run(c, ref.AA, [("f", ref.ASC)], 200)
    zeros = [v for _, v, _ in hits if v == 0.0]
    signs = [math.copysign(1.0, v) for v in zeros]
    assert signs == [-1.0] * 30 + [1.0] * 30


def test_corpus_lengths_are_exact_under_fieldnorm():
    for c in (ref.tied_corpus(), ref.classes_corpus(), ref.edge_corpus(129)):
        assert (ref.quantize_lengths(c.lengths) == c.lengths).all()
    # the decode table restated here agrees with the writer's encoder
    from quickwit_amd.fieldnorm import norm_to_id
    import numpy as np
    lens = np.arange(0, 300)
    ids = norm_to_id(lens)
    assert [ref.fieldnorm_decode(int(i)) for i in ids] == \
        ref.quantize_lengths(lens).tolist()
