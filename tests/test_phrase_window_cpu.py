"""Sloppy phrases and multi-token phrase prefixes, the parts that need no
GPU: the brute-force reference (tests/phrase_window_reference.py) against
the recorded vectors, the REST shim's AST shapes for the eleven es_compat_extra
golden steps that use these forms, and the CPU oracle, which has no
evaluator for them and must keep refusing them rather than match as slop 0.
"""
import json
import os
import random

import pytest

import phrase_window_reference as ref
from quickwit_amd import splitgen
from quickwit_amd.rest import es_query_to_ast

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_STEPS = [22, 77, 78, 79, 81, 82, 89, 92, 93, 97, 98]


def load_vectors():
    with open(os.path.join(REPO, "tests", "golden",
                           "phrase_window_vectors.json")) as f:
        return json.load(f)


def load_steps():
    with open(os.path.join(REPO, "tests", "golden",
                           "rest_scenarios.json")) as f:
        return json.load(f)["suites"]["es_compat_extra"]


# ------------------------------------------------------------- reference
def test_reference_reproduces_slop_vectors():
    v = load_vectors()
    for group in ("slop_queries", "transposition"):
        docs = [ref.tokens(d) for d in v[group]["docs"]]
        for c in v[group]["cases"]:
            got = ref.slop_hits(docs, ref.tokens(c["phrase"]), c["slop"])
            assert len(got) == c["count"], (c, got)


def test_reference_reproduces_prefix_vector():
    v = load_vectors()["prefix_max_expansions"]
    docs = [ref.tokens(d) for d in v["docs"]]
    for c in v["cases"]:
        got = ref.prefix_hits(docs, ref.tokens(c["phrase"]),
                              c["max_expansions"])
        assert len(got) == c["count"], (c, got)
    # uncapped, the same prefix reaches all three
    assert len(ref.prefix_hits(docs, ["fantasy", "some"], 50)) == 3


def test_reference_tokens_agree_with_the_writer():
    v = load_vectors()
    for group in v.values():
        if isinstance(group, dict):
            for d in group["docs"]:
                assert ref.tokens(d) == splitgen.tokenize(d, "default"), d


def test_reference_dp_equals_exhaustive_choice():
    rng = random.Random(5)
    vocab = ["a", "b", "c"]
    for _ in range(400):
        doc = [rng.choice(vocab) for _ in range(rng.randint(1, 7))]
        phrase = [rng.choice(vocab) for _ in range(rng.randint(2, 4))]
        assert ref.min_slop(doc, phrase) == \
            ref.min_slop_exhaustive(doc, phrase), (doc, phrase)


def test_reference_definition_corner_cases():
    # a transposition costs 2; chosen positions need not be distinct
    assert ref.min_slop(["b", "a"], ["a", "b"]) == 2
    assert ref.min_slop(["beta"], ["beta", "beta"]) == 1
    assert ref.min_slop(["x"], ["x", "y"]) is None


# ------------------------------------------------------------- REST shapes
def pp(field, phrase, lenient=False, max_expansions=50):
    return {"type": "phrase_prefix", "field": field, "phrase": phrase,
            "max_expansions": max_expansions,
            "params": {"mode": {"type": "phrase"}}, "lenient": lenient}


MSG = "payload.commits.message"
PRB = "payload.pull_request.body"
MULTI = [MSG, "payload.description", "payload.comment.body"]
EXPECTED_AST = {
    22: {"type": "full_text", "field": MSG, "text": "zone explosion",
         "params": {"mode": {"type": "phrase", "slop": 1}}},
    77: pp(PRB, "to p"),
    78: pp(PRB, "be to p"),
    79: pp(MSG, "automated comm"),
    # analyzer raw: one token, the uncapped prefix path
    81: {"type": "wildcard", "field": MSG, "value": "automated comm*"},
    82: ValueError,  # unknown analyzer: 400
    89: {"type": "full_text", "field": MSG, "text": "zone explosion",
         "params": {"mode": {"type": "phrase", "slop": 1}}},
    92: pp(MSG, "zone of expl"),
    93: pp(MSG, "zone of expl", lenient=True),
    97: {"type": "bool",
         "should": [pp(f, "to be", lenient=True) for f in MULTI]},
    98: {"type": "bool",
         "should": [pp(f, "to b", lenient=True) for f in MULTI]},
}


@pytest.mark.parametrize("step", GOLDEN_STEPS)
def test_rest_shim_ast_of_golden_step(step):
    body = load_steps()[step]["json"]
    exp = EXPECTED_AST[step]
    if exp is ValueError:
        assert load_steps()[step]["status_code"] == 400
        with pytest.raises(ValueError):
            es_query_to_ast(body["query"])
        return
    assert es_query_to_ast(body["query"]) == exp


def test_rest_shim_phrase_prefix_details():
    q = {"match_phrase_prefix": {"body": {"query": "quick brown f",
                                          "max_expansions": 7, "slop": 3}}}
    ast = es_query_to_ast(q)
    assert ast == pp("body", "quick brown f", max_expansions=7)
    # one analyzed token stays the wildcard form, whatever max_expansions
    q1 = {"match_phrase_prefix": {"body": {"query": "fix",
                                           "max_expansions": 2}}}
    assert es_query_to_ast(q1) == {"type": "wildcard", "field": "body",
                                   "value": "fix*"}
    # unknown fields of a multi_match contribute nothing
    schema = {"fields": [{"name": "body", "type": "text",
                          "tokenizer": "default"}]}
    mm = {"multi_match": {"fields": ["body", "nope"], "query": "a b",
                          "type": "phrase", "slop": 2}}
    assert es_query_to_ast(mm, schema) == {
        "type": "full_text", "field": "body", "text": "a b",
        "params": {"mode": {"type": "phrase", "slop": 2}}}


# ------------------------------------------------------------- the oracle
SCHEMA = {"timestamp_field": None, "fields": [
    {"name": "body", "type": "text", "tokenizer": "default",
     "record": "position", "fieldnorms": True}]}


@pytest.fixture(scope="module")
def oracle():
    import __graft_entry__
    __graft_entry__.build()
    from quickwit_amd.api import OracleSearcher
    w = splitgen.SplitWriter(SCHEMA, "pw", store_docs=False)
    w.add_documents([{"body": "alpha beta"}, {"body": "alpha gamma beta"},
                     {"body": "alpha betamax"}])
    cpu = OracleSearcher()
    cpu.add_split("pw", w.finalize())
    return cpu


@pytest.mark.parametrize("query", [
    {"type": "full_text", "field": "body", "text": "alpha beta",
     "params": {"mode": {"type": "phrase", "slop": 1}}},
    pp("body", "alpha bet"),
    {"type": "user_input", "user_text": 'body:"alpha bet"*',
     "default_fields": ["body"]},
], ids=["slop1", "phrase_prefix_ast", "grammar_prefix"])
def test_oracle_refuses_and_does_not_match(oracle, query):
    from quickwit_amd.api import make_leaf_request
    r = oracle.leaf_search(make_leaf_request(query, SCHEMA, [("pw", 3)],
                                             max_hits=3))
    assert r.get("failed_splits"), r
    assert r.get("num_hits", 0) == 0
    assert "not supported" in r["failed_splits"][0]["error"]
