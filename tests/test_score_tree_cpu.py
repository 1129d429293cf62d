"""Proves tests/score_tree_reference.py — the float64 scores of boolean
trees, their match sets and the ordering — against the oracle, before a GPU
is involved, on every case test_score_tree_gpu.py uses.

It also asserts, from the reference alone, the condition the comparison rule
rests on: any two matching docs of a case whose float64 scores differ, differ
by more than 1e-4 relative (ten times the tolerance), so no tolerance can
blur the edge between two tie groups. That is a condition on the corpus, not
a tolerance on the code under test.
"""
import pytest

import score_tree_reference as ref
from quickwit_amd.api import OracleSearcher, make_leaf_request


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def oracle():
    c = ref.corpus()
    s = OracleSearcher()
    s.add_split(c.split_id, c.data)
    return s


def run(oracle, node, sort, max_hits):
    c = ref.corpus()
    req = make_leaf_request(node, ref.SCHEMA, [(c.split_id, c.num_docs)],
                            max_hits=max_hits,
                            sort_fields=ref.tr.sort_fields(sort))
    r = oracle.leaf_search(req)
    assert not r.get("failed_splits"), r.get("failed_splits")
    return r


@pytest.mark.parametrize("name,node", ref.CASES, ids=[n for n, _ in ref.CASES])
def test_reference_matches_oracle(oracle, name, node):
    c = ref.corpus()
    n, full = ref.ranked(c, node, ref.SCORE_DESC)
    assert n > 0, name
    r = run(oracle, node, ref.SCORE_DESC, c.num_docs)
    assert r.get("num_hits", 0) == n, name
    ref.compare(ref.hits_of(r), full, 0, c.num_docs, name)
    # a page that ends inside the list
    r = run(oracle, node, ref.SCORE_DESC, 100)
    ref.compare(ref.hits_of(r), full, 0, 100, (name, 100))


@pytest.mark.parametrize("name,node", ref.CASES, ids=[n for n, _ in ref.CASES])
def test_distinct_scores_are_far_apart(name, node):
    assert ref.min_score_gap(ref.corpus(), node) > ref.GAP, name
    assert ref.min_score_gap(ref.second_segment(), node) > ref.GAP, name


def test_downstream_sorts_match_oracle(oracle):
    c = ref.corpus()
    for sort in (ref.SCORE_ASC, [("u", ref.DESC), ("_score", ref.DESC)]):
        n, full = ref.ranked(c, ref.OR_OF_ANDS, sort)
        r = run(oracle, ref.OR_OF_ANDS, sort, c.num_docs)
        assert r.get("num_hits", 0) == n
        ref.compare(ref.hits_of(r), full, 0, c.num_docs, sort)


def test_corpus_has_the_shapes_the_gpu_test_needs():
    c = ref.corpus()
    n = c.num_docs
    assert n == 2 * ref.TILE_DOCS + 37
    df = {w: int((c.tf(w) > 0).sum()) for w in ref.WORDS}
    assert abs(df["a"] - n / 2) < n / 8  # dense: blocks straddle both edges
    assert df["x"] < 128  # one short posting block
    mid = c.tf("m")[ref.TILE_DOCS:2 * ref.TILE_DOCS]
    assert not mid.any() and c.tf("m")[:ref.TILE_DOCS].any() \
        and c.tf("m")[2 * ref.TILE_DOCS:].any()
    assert ref.ABSENT not in c.vocab
    # the gate matters: docs with 'b' but not 'c' match the core case and
    # must not get the 'b' score
    m, s = ref.evaluate(c, ref.CASES[0][1])
    _, sa = ref.evaluate(c, ref.term("a"))
    b_only = m & (c.tf("b") > 0) & (c.tf("c") == 0)
    assert b_only.any() and (s[b_only] == sa[b_only]).all()
    # the search_after cursor of the GPU test sits in an exact two-term group
    _, full = ref.ranked(c, ref.OR_OF_ANDS, ref.SCORE_DESC)
    top = [d for d, _, k in full if k == full[0][2]]
    assert len(top) == 5 and (c.tf("a")[top] == 0).all()
