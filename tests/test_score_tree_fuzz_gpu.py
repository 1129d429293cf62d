"""Seeded random SCORED boolean trees, GPU <-> oracle (deterministic).

Sixty trees of depth up to 3 over the synthetic hdfs-logs split, all sorted
by _score: term, range and match_all leaves, boosts in [0.5, 2],
minimum_should_match in {unset, 0, 1} on bools with a nested bool clause and
up to 2 on bools of plain clauses whose shoulds are terms. The generator
emits none of the classes that stay refused (const-score nodes,
minimum_should_match > 1 over nested clauses, non-positive boosts), so the
product must answer every query: zero refusals is asserted. QW_FUZZ_SEED
offsets the seed.

Parity rule (the one of test_fuzz_parity.py): num_hits equal, scores within
1e-5 relative pointwise, ids set-equal within rounded tie groups except
possibly the truncated boundary group.
"""
import math
import os
import random

import pytest

from quickwit_amd import splitgen
from quickwit_amd.api import GpuSearcher, OracleSearcher, make_leaf_request

pytestmark = pytest.mark.gpu

NDOCS = 20_000
SID = "score-tree-fuzz"
SCHEMA = splitgen.HDFS_SCHEMA
N_QUERIES = 60
SCORE_SORT = [{"field_name": "_score", "sort_order": 1}]


@pytest.fixture(scope="module")
def searchers():
    import __graft_entry__
    __graft_entry__.build()
    data = splitgen.generate_split(0, NDOCS, seed=404)
    gpu, cpu = GpuSearcher(device=0), OracleSearcher()
    gpu.add_split(SID, data)
    cpu.add_split(SID, data)
    return gpu, cpu


def maybe_boost(rng, node):
    if rng.random() < 0.3:
        return {"type": "boost", "underlying": node,
                "boost": round(rng.uniform(0.5, 2.0), 3)}
    return node


def rand_term(rng):
    # mostly frequent words, so that nested clauses match something; one
    # term in ten is missing from the dictionary
    field, pool = rng.choice([
        ("body", ["w%05d" % rng.randrange(0, 40)] * 6 +
                 ["w%05d" % rng.randrange(0, 2000)] * 3 +
                 ["zz_absent_%d" % rng.randrange(3)]),
        ("body", ["w%05d" % rng.randrange(0, 40)]),
        ("severity_text", ["DEBUG", "INFO", "WARN", "ERROR", "FATAL"] * 2 +
                          ["nope"]),
    ])
    return maybe_boost(rng, {"type": "term", "field": field,
                             "value": rng.choice(pool)})


def rand_range(rng):
    lo = rng.randrange(0, 900)
    return {"type": "range", "field": "tenant_id",
            "lower_bound": {"included": lo},
            "upper_bound": {"included": lo + rng.randrange(1, 400)}}


def rand_clause(rng, depth):
    r = rng.random()
    if r < 0.5:
        return rand_term(rng)
    if r < 0.62:
        return rand_range(rng)
    if r < 0.67:
        return {"type": "match_all"}
    if depth < 3:
        return rand_bool(rng, depth + 1)
    return rand_term(rng)


def rand_bool(rng, depth=1):
    b = {"type": "bool"}
    for occ, pmax in (("must", 2), ("should", 3), ("filter", 1),
                      ("must_not", 1)):
        n = rng.randrange(1, pmax + 1) if rng.random() < 0.55 else 0
        if n:
            b[occ] = [rand_clause(rng, depth) for _ in range(n)]
    if not any(k in b for k in ("must", "should", "filter")):
        b["should"] = [rand_term(rng) for _ in range(rng.randrange(1, 4))]
    shoulds = b.get("should", [])
    if shoulds and rng.random() < 0.5:
        # up to 2 only where the shoulds are plain terms and no clause of
        # this bool, in any position, is a bool itself
        def kind(c):
            return kind(c["underlying"]) if c["type"] == "boost" else c["type"]
        clauses = [c for occ in ("must", "should", "filter", "must_not")
                   for c in b.get(occ, [])]
        top = 2 if (all(kind(c) == "term" for c in shoulds) and
                    all(kind(c) != "bool" for c in clauses)) else 1
        b["minimum_should_match"] = rng.randrange(0, top + 1)
    return maybe_boost(rng, b)


def scores_of(hits):
    return [h.get("sort_value", {}).get("f64") for h in hits]


def assert_parity(g, e, label):
    assert g.get("num_hits", 0) == e.get("num_hits", 0), label
    gh, eh = g.get("partial_hits", []), e.get("partial_hits", [])
    assert len(gh) == len(eh), label
    for a, b in zip(scores_of(gh), scores_of(eh)):
        if a is None or b is None:
            assert a == b, label
        else:
            assert math.isclose(a, b, rel_tol=1e-5, abs_tol=1e-9), label

    def grp(hits):
        out = {}
        for h in hits:
            s = h.get("sort_value", {}).get("f64")
            out.setdefault(None if s is None else round(s, 4),
                           set()).add(h.get("doc_id", 0))
        return out
    gg, ee = grp(gh), grp(eh)
    keys = sorted((k for k in gg if k is not None), reverse=True)
    for k in keys[:-1]:
        assert gg[k] == ee.get(k), (label, k)


def test_random_scored_trees_match_oracle(searchers):
    gpu, cpu = searchers
    rng = random.Random(9090 + int(os.environ.get("QW_FUZZ_SEED", "0")))
    gated0 = 0
    try:
        gated0 = gpu.kernel_stats("union_bm25_gated")[1]
    except KeyError:
        pass
    refused = []
    for qi in range(N_QUERIES):
        q = rand_bool(rng)
        mh = rng.choice([7, 50, 200])
        req = make_leaf_request(q, SCHEMA, [(SID, NDOCS)], max_hits=mh,
                                sort_fields=SCORE_SORT)
        label = f"q{qi}: {q} max_hits={mh}"
        g, e = gpu.leaf_search(req), cpu.leaf_search(req)
        assert not e.get("failed_splits"), (label, e.get("failed_splits"))
        if g.get("failed_splits"):
            refused.append((label, g["failed_splits"][0].get("error", "")))
            continue
        assert_parity(g, e, label)
    assert not refused, refused
    # the battery must really reach the gated kernel
    gated = gpu.kernel_stats("union_bm25_gated")[1] - gated0
    print(f"{gated} of {N_QUERIES} queries ran the gated kernel")
    assert gated >= 1
