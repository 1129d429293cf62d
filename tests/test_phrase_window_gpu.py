"""Sloppy phrases and multi-token phrase prefixes on the device
(k_phrase_window_bitmap), id-exact against the brute force of
tests/phrase_window_reference.py. Small corpora, max_hits = the corpus size.
"""
import json
import os
import random

import pytest

import phrase_window_reference as ref
from quickwit_amd import splitgen
from quickwit_amd.api import make_leaf_request

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMA = {"timestamp_field": None, "fields": [
    {"name": "body", "type": "text", "tokenizer": "default",
     "record": "position", "fieldnorms": True}]}
VOCAB = ["alpha", "beta", "gamma", "delta", "eps", "zeta"]
SLOPS = [1, 2, 3, 7, 31]
P8A = ["alpha", "beta", "gamma", "delta", "eps", "zeta", "alpha", "beta"]
P8B = ["beta", "alpha", "beta", "alpha", "gamma", "gamma", "delta", "beta"]
PHRASES = [["alpha", "beta"], ["beta", "beta"], ["gamma", "delta", "eps"],
           ["zeta", "alpha", "zeta"], ["eps", "eps", "eps", "eps"],
           ["delta", "gamma", "beta", "alpha"], P8A, P8B]


def spread(phrase, gaps):
    """The phrase with a filler word put in before token g, for g in gaps:
    each one costs 1."""
    out = []
    for i, t in enumerate(phrase):
        out += ["filler"] * gaps.count(i) + [t]
    return out


def corpus():
    """test_phrase.py's shape (frequent terms span several 128-posting
    blocks, tf > 1), plus long docs so that large slops still add matches,
    docs whose match sits at position 0 (the window reaches below zero),
    8-token phrases spread by 0..3 fillers, and docs of length 1."""
    rng = random.Random(1234)
    docs = [[rng.choice(VOCAB) for _ in range(rng.randint(3, 12))]
            for _ in range(700)]
    docs += [[rng.choice(VOCAB) for _ in range(rng.randint(30, 60))]
             for _ in range(40)]
    docs += [["beta", "alpha", "gamma"], ["beta", "alpha"],
             ["gamma", "beta", "alpha", "delta"], ["delta", "gamma", "alpha"]]
    for p8 in (P8A, P8B):
        docs += [spread(p8, []), spread(p8, [4]), spread(p8, [2, 6]),
                 spread(p8, [1, 1, 5]), spread(p8, [3, 3, 3, 7])]
    docs += [[w] for w in VOCAB[:4]]
    return docs


DOCS = corpus()
NDOCS = len(DOCS)
EXPECTED = {(tuple(p), s): ref.slop_hits(DOCS, p, s)
            for p in PHRASES for s in [0] + SLOPS}
CASES = [(p, s) for p in PHRASES for s in SLOPS]

# the case selection, judged by the reference alone at collection time:
# every case has a non-empty proper subset of the corpus, and at least half
# of them differ from the same phrase at the next smaller slop of [0]+SLOPS
_differ = 0
for _p, _s in CASES:
    _e = EXPECTED[(tuple(_p), _s)]
    assert 0 < len(_e) < NDOCS, (_p, _s, len(_e))
    _prev = ([0] + SLOPS)[SLOPS.index(_s)]
    _differ += _e != EXPECTED[(tuple(_p), _prev)]
assert 2 * _differ >= len(CASES), (_differ, len(CASES))


def make_split(docs_toks, split_id, schema=SCHEMA):
    w = splitgen.SplitWriter(schema, split_id, store_docs=False)
    w.add_documents([{"body": " ".join(t)} for t in docs_toks])
    return w.finalize()


def slop_query(toks, slop):
    mode = {"type": "phrase"}
    if slop:
        mode["slop"] = slop
    return {"type": "full_text", "field": "body", "text": " ".join(toks),
            "params": {"mode": mode}}


def prefix_query(toks, max_expansions=50, **extra):
    q = {"type": "phrase_prefix", "field": "body", "phrase": " ".join(toks),
         "max_expansions": max_expansions,
         "params": {"mode": {"type": "phrase"}}, "lenient": False}
    q.update(extra)
    return q


def search(gpu, query, splits, schema=SCHEMA, **kw):
    return gpu.leaf_search(make_leaf_request(query, schema, splits, **kw))


def hit_ids(r):
    return sorted(h.get("doc_id", 0) for h in r.get("partial_hits", []))


def check(gpu, query, split, ndocs, expected):
    r = search(gpu, query, [(split, ndocs)], max_hits=ndocs)
    assert not r.get("failed_splits"), r.get("failed_splits")
    assert r.get("num_hits", 0) == len(expected), query
    assert hit_ids(r) == expected, query


@pytest.fixture(scope="module")
def gpu():
    import __graft_entry__
    __graft_entry__.build()
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)
    g.add_split("pw", make_split(DOCS, "pw"))
    return g


# ---------------------------------------------------------------- vectors
def test_golden_vectors(gpu):
    with open(os.path.join(REPO, "tests", "golden",
                           "phrase_window_vectors.json")) as f:
        v = json.load(f)
    for name in ("slop_queries", "transposition", "prefix_max_expansions"):
        texts = v[name]["docs"]
        docs = [ref.tokens(t) for t in texts]
        w = splitgen.SplitWriter(SCHEMA, "v-" + name, store_docs=False)
        w.add_documents([{"body": t} for t in texts])
        gpu.add_split("v-" + name, w.finalize())
        for c in v[name]["cases"]:
            toks = ref.tokens(c["phrase"])
            if "max_expansions" in c:
                exp = ref.prefix_hits(docs, toks, c["max_expansions"])
                queries = [prefix_query(toks, c["max_expansions"])]
            else:
                exp = ref.slop_hits(docs, toks, c["slop"])
                # the query grammar on the field and the full_text phrase
                # mode; with a slop also the reference's own form, the
                # grammar over the default field
                queries = [{"type": "user_input",
                            "user_text": "body:" + c["query"],
                            "default_fields": None},
                           slop_query(toks, c["slop"])]
                if c["slop"]:
                    queries.append({"type": "user_input",
                                    "user_text": c["query"],
                                    "default_fields": ["body"]})
            assert len(exp) == c["count"], c
            for q in queries:
                check(gpu, q, "v-" + name, len(docs), exp)


# ------------------------------------------------------ randomised corpus
@pytest.mark.parametrize(
    "toks,slop", CASES,
    ids=["%d_%s~%d" % (len(p), "".join(t[0] for t in p), s)
         for p, s in CASES])
def test_slop_matches_brute_force(gpu, toks, slop):
    check(gpu, slop_query(toks, slop), "pw", NDOCS,
          EXPECTED[(tuple(toks), slop)])


def test_query_grammar_forms(gpu):
    check(gpu, {"type": "user_input", "user_text": 'body:"gamma delta eps"~3',
                "default_fields": None}, "pw", NDOCS,
          EXPECTED[(("gamma", "delta", "eps"), 3)])
    check(gpu, {"type": "user_input", "user_text": 'body:"gamma delta e"*',
                "default_fields": None}, "pw", NDOCS,
          ref.prefix_hits(DOCS, ["gamma", "delta", "e"]))
    # one token: slop is ignored, the phrase is a plain term
    check(gpu, slop_query(["alpha"], 3), "pw", NDOCS,
          [d for d, t in enumerate(DOCS) if "alpha" in t])


# ------------------------------------------------------ ordering and cache
def test_slop_order_and_prefix_do_not_share_cache_entries(gpu):
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)  # a searcher of its own: a cold hitset cache
    g.add_split("pw", make_split(DOCS, "pw"))
    toks = ["zeta", "alpha", "zeta"]
    for slop in (0, 1, 2, 2, 1, 0):
        check(g, slop_query(toks, slop), "pw", NDOCS,
              EXPECTED[(tuple(toks), slop)])
    pre = ["gamma", "delta"]  # "delta" is both a term and a prefix
    plain = ref.slop_hits(DOCS, pre, 0)
    for _ in range(2):
        check(g, prefix_query(pre), "pw", NDOCS, ref.prefix_hits(DOCS, pre))
        check(g, slop_query(pre, 0), "pw", NDOCS, plain)
        check(g, prefix_query(["gamma", "d"]), "pw", NDOCS,
              ref.prefix_hits(DOCS, ["gamma", "d"]))
        check(g, prefix_query(["gamma", "d"], 0), "pw", NDOCS, [])


# ------------------------------------------------------------------ limits
def test_limits(gpu):
    r = search(gpu, slop_query(["alpha", "beta"], 32), [("pw", NDOCS)])
    assert r.get("failed_splits") and r.get("num_hits", 0) == 0
    assert "slop > 31 not supported" in r["failed_splits"][0]["error"]

    nine = P8A + ["gamma"]
    for q in (slop_query(nine, 1), prefix_query(nine)):
        r = search(gpu, q, [("pw", NDOCS)])
        assert r.get("failed_splits") and r.get("num_hits", 0) == 0, q
        assert "8 tokens" in r["failed_splits"][0]["error"]

    schema_nf = {"timestamp_field": None, "fields": [
        {"name": "body", "type": "text", "tokenizer": "default",
         "record": "freq", "fieldnorms": True}]}
    gpu.add_split("pw-nf", make_split([["alpha", "beta"]], "pw-nf", schema_nf))
    for q in (slop_query(["alpha", "beta"], 1), prefix_query(["alpha", "be"])):
        r = search(gpu, q, [("pw-nf", 1)], schema=schema_nf)
        assert r.get("failed_splits"), q
        assert "position" in r["failed_splits"][0]["error"]

    # an absent token, in the middle or in front of the prefix: no hit
    check(gpu, slop_query(["alpha", "missingtok", "beta"], 7), "pw", NDOCS, [])
    check(gpu, prefix_query(["alpha", "missingtok", "be"]), "pw", NDOCS, [])

    score = [{"field_name": "_score", "sort_order": 1}]
    for q in (slop_query(["alpha", "beta"], 1), prefix_query(["alpha", "be"])):
        r = search(gpu, q, [("pw", NDOCS)], max_hits=5, sort_fields=score)
        assert r.get("failed_splits"), q  # const-score: rejected, not scored


def test_phrase_prefix_ast_edges(gpu):
    # zero tokens: match_none, or match_all under zero_terms_query: all
    check(gpu, prefix_query([]), "pw", NDOCS, [])
    q = prefix_query([])
    q["params"]["zero_terms_query"] = "all"
    check(gpu, q, "pw", NDOCS, list(range(NDOCS)))
    # a missing field: match_none when lenient, an error otherwise
    q = prefix_query(["alpha", "be"], lenient=True, field="nope")
    check(gpu, q, "pw", NDOCS, [])
    r = search(gpu, prefix_query(["alpha", "be"], field="nope"),
               [("pw", NDOCS)])
    assert r.get("failed_splits")
    # one token: an uncapped prefix whatever max_expansions says
    check(gpu, prefix_query(["ga"], 0), "pw", NDOCS,
          [d for d, t in enumerate(DOCS) if "gamma" in t])


# ---------------------------------------------------- phrase-prefix corpus
def prefix_corpus():
    """71 last-token terms share the prefix "pre" ("pre" itself and
    pre00..pre69), so max_expansions 1, 50 and 70 each cut the expansion
    list somewhere else; pre03 follows "lead" in more than 128 docs (an
    expansion spanning two posting blocks)."""
    rng = random.Random(99)
    tails = ["pre"] + ["pre%02d" % i for i in range(70)]
    docs = []
    for i in range(900):
        tail = "pre03" if i % 4 == 0 else rng.choice(tails)
        kind = rng.randint(0, 5)
        if kind == 0:
            docs.append(["other", tail])
        elif kind == 1:
            docs.append(["lead", "gap", tail])
        elif kind == 2:
            docs.append(["go", "lead", tail, "lead"])
        else:
            docs.append(["lead", tail])
    docs.append(["lead", "pre69"])  # the 71st term: past every tested cap
    return docs


def test_phrase_prefix_expansion_caps(gpu):
    docs = prefix_corpus()
    n = len(docs)
    gpu.add_split("pp", make_split(docs, "pp"))
    assert sum(1 for t in docs if "pre03" in t) > 128
    seen = set()
    for me in (1, 50, 70, 100):
        assert len(ref.expansions(docs, "pre", me)) == min(me, 71)
        exp = ref.prefix_hits(docs, ["lead", "pre"], me)
        assert exp and tuple(exp) not in seen  # every cap cuts elsewhere
        seen.add(tuple(exp))
        check(gpu, prefix_query(["lead", "pre"], me), "pp", n, exp)
        check(gpu, prefix_query(["go", "lead", "pre"], me), "pp", n,
              ref.prefix_hits(docs, ["go", "lead", "pre"], me))
    # the prefix is a whole term with further expansions behind it
    check(gpu, prefix_query(["lead", "pre03"]), "pp", n,
          ref.prefix_hits(docs, ["lead", "pre03"]))
    # no expansion at all
    assert not ref.expansions(docs, "qq", 50)
    check(gpu, prefix_query(["lead", "qq"]), "pp", n, [])


# ------------------------------------------------------------- composition
def test_both_forms_inside_bool(gpu):
    sl = set(EXPECTED[(("alpha", "beta"), 2)])
    pf = set(ref.prefix_hits(DOCS, ["gamma", "de"]))
    with_z = {d for d, t in enumerate(DOCS) if "zeta" in t}
    zeta = {"type": "term", "field": "body", "value": "zeta"}
    for form, hits in ((slop_query(["alpha", "beta"], 2), sl),
                       (prefix_query(["gamma", "de"]), pf)):
        check(gpu, {"type": "bool", "filter": [form], "must": [zeta]},
              "pw", NDOCS, sorted(hits & with_z))
        check(gpu, {"type": "bool", "must": [form, zeta]},
              "pw", NDOCS, sorted(hits & with_z))
        check(gpu, {"type": "bool", "must": [zeta], "must_not": [form]},
              "pw", NDOCS, sorted(with_z - hits))
    check(gpu, {"type": "bool", "must": [slop_query(["alpha", "beta"], 2),
                                         prefix_query(["gamma", "de"])]},
          "pw", NDOCS, sorted(sl & pf))


def test_multi_segment_split(gpu):
    a, b = DOCS[:400], DOCS[400:]
    data = splitgen.concat_segments(
        [make_split(a, "ms"), make_split(b, "ms")], "ms")
    gpu.add_split("ms", data)
    for q, fn in ((slop_query(["zeta", "alpha", "zeta"], 3),
                   lambda d: ref.slop_hits(d, ["zeta", "alpha", "zeta"], 3)),
                  (prefix_query(["gamma", "de"]),
                   lambda d: ref.prefix_hits(d, ["gamma", "de"]))):
        r = search(gpu, q, [("ms", NDOCS)], max_hits=NDOCS)
        assert not r.get("failed_splits"), r.get("failed_splits")
        got = sorted((h.get("segment_ord", 0), h.get("doc_id", 0))
                     for h in r.get("partial_hits", []))
        exp = [(0, d) for d in fn(a)] + [(1, d) for d in fn(b)]
        assert exp and got == exp, q


def test_split_without_positions_fails_alone(gpu):
    schema_nf = {"timestamp_field": None, "fields": [
        {"name": "body", "type": "text", "tokenizer": "default",
         "record": "freq", "fieldnorms": True}]}
    gpu.add_split("sa", make_split([["alpha", "x", "beta"],
                                    ["beta", "alpha"]], "sa"))
    gpu.add_split("sb", make_split([["alpha", "beta"]], "sb", schema_nf))
    for q in (slop_query(["alpha", "beta"], 1), prefix_query(["x", "be"])):
        r = search(gpu, q, [("sa", 2), ("sb", 1)], max_hits=5)
        assert r["num_hits"] == 1 and hit_ids(r) == [0], q
        fails = r.get("failed_splits", [])
        assert len(fails) == 1 and fails[0]["split_id"] == "sb"
        assert "position" in fails[0]["error"]
        assert r.get("num_successful_splits", 0) == 1


# -------------------------------------------------------------------- REST
def test_rest_es_compat_extra_without_phrase_skips(gpu):
    from fastapi.testclient import TestClient

    from quickwit_amd.api import GpuSearcher
    from quickwit_amd.rest import create_app
    from rest_replay import replay_suite

    def skip_only_stats_and_regexp(i, step):
        if step.get("endpoint") == "_stats":
            return "global _stats totals depend on cross-suite session state"
        body = step.get("json")
        if isinstance(body, dict) and "regexp" in (body.get("query") or {}):
            return "regex queries: declared out"
        return None

    with open(os.path.join(REPO, "tests", "golden",
                           "rest_scenarios.json")) as f:
        steps = json.load(f)["suites"]["es_compat_extra"]
    client = TestClient(create_app(lambda: GpuSearcher(device=0)))
    ran, skipped = replay_suite(client, steps, skip_only_stats_and_regexp)
    assert ran >= 129, (ran, skipped)
    assert len(skipped) <= 2, skipped
