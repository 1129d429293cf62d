"""Regex queries on the device: k_dict_dfa_match scans the field's term
dictionary, k_terms_union_bitmap ORs the matched terms' postings. Ids are
compared exactly (max_hits = corpus size) with tests/regex_reference.py
(Python's re.fullmatch over the term set, independent of csrc/qregex.h)."""
import json
import os

import pytest

import regex_reference as ref
from quickwit_amd import splitgen
from quickwit_amd.api import make_leaf_request

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_DOCS = 8192  # gpu_types.h
SCHEMA = {"timestamp_field": None, "fields": [
    {"name": "n", "type": "u64", "fast": True},
    {"name": "k", "type": "str", "fast": True},
    {"name": "tag", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": True},
    {"name": "body", "type": "text", "tokenizer": "default",
     "record": "position", "fieldnorms": True}]}


def regex(pattern, field="body"):
    return {"type": "regex", "field": field, "regex": pattern}


def term(value, field="body"):
    return {"type": "term", "field": field, "value": value}


def make_split(docs, split_id):
    """docs: token lists -> body; doc d also gets n = d % 7, k = "k<d % 3>"."""
    w = splitgen.SplitWriter(SCHEMA, split_id, store_docs=False)
    w.add_documents([{"body": " ".join(t), "n": d % 7, "k": "k%d" % (d % 3)}
                     for d, t in enumerate(docs)])
    return w.finalize()


def search(gpu, query, splits, **kw):
    return gpu.leaf_search(make_leaf_request(query, SCHEMA, splits, **kw))


def hit_ids(r):
    return sorted(h.get("doc_id", 0) for h in r.get("partial_hits", []))


def check(gpu, query, split, ndocs, expected):
    r = search(gpu, query, [(split, ndocs)], max_hits=ndocs)
    assert not r.get("failed_splits"), r.get("failed_splits")
    assert r.get("num_hits", 0) == len(expected), query
    assert hit_ids(r) == expected, query


def launches(gpu, name):
    return gpu.kernel_stats(name)[1]


# ------------------------------------------------------- dictionary corpora
SPECIAL = ["a", "x" * 40, "日本", "éa5"]  # 1 byte, 40 bytes, multi-byte


def dict_docs(n_terms):
    """A corpus whose body field has exactly n_terms distinct terms; every
    fifth doc has an empty body, so no pattern can select every doc."""
    if n_terms == 1:
        terms = ["w0005"]
    else:
        terms = SPECIAL + ["w%04d" % i for i in range(n_terms - len(SPECIAL))]
    docs = []
    for i in range(max(n_terms, 40)):
        docs.append([terms[i % n_terms], terms[(7 * i + 3) % n_terms]])
        if i % 4 == 0:
            docs.append([])
    assert len(ref.term_set(docs)) == n_terms
    return docs


DICT_SIZES = [1, 63, 64, 65, 3000]
DICT_DOCS = {n: dict_docs(n) for n in DICT_SIZES}
# the first three tables are staged in LDS, BIG_TABLE is read from global
# memory: tests/test_regex_cpu.py::test_table_sizes_cover_both_scan_paths
BIG_TABLE = ref.BIG_TABLE
DICT_PATTERNS = ref.SMALL_TABLES + [BIG_TABLE]
DICT_EXPECTED = {}
for _n, _docs in DICT_DOCS.items():
    for _p in (DICT_PATTERNS if _n > 1 else ["w.*[05]"]):
        _terms = ref.term_set(_docs)
        _m = ref.matched_terms(_p, _terms)
        # one term cannot have a non-empty proper subset: docs only there
        assert 0 < len(_m) and (len(_m) < len(_terms) or _n == 1), (_n, _p)
        _h = ref.regex_hits(_docs, _p)
        assert 0 < len(_h) < len(_docs), (_n, _p)
        DICT_EXPECTED[(_n, _p)] = _h


# ------------------------------------------------------------ union corpus
def union_docs():
    """num_docs = TILE_DOCS + 37 (no multiple of 32). u<df> terms have that
    df; p* terms sit on the named doc ids; doc 5 carries 120 c-terms; 5000
    m-terms have df 1-2; every doc also has "zz", which no pattern matches."""
    n = TILE_DOCS + 37
    docs = [["zz"] for _ in range(n)]
    for df, step, start in ((1, 1, 7), (127, 3, 1), (128, 5, 2), (129, 7, 3),
                            (400, 11, 4)):
        for i in range(df):
            docs[(start + i * step) % n].append("u%d" % df)
    for name, d in (("pa", 0), ("pb", 31), ("pc", 32), ("pd", TILE_DOCS - 1),
                    ("pe", TILE_DOCS), ("pf", n - 1)):
        docs[d].append(name)
    docs[5] += ["c%03d" % i for i in range(120)]
    for i in range(5000):
        docs[(i * 13 + 40) % n].append("m%04d" % i)
        if i % 3 == 0:
            docs[(i * 29 + 4100) % n].append("m%04d" % i)
    return docs


UDOCS = union_docs()
UN = len(UDOCS)
UNION_PATTERNS = ["u1", "u127", "u128", "u129", "u400", "u12[789]", "u.*",
                  "p[a-f]", "pa|pf", "c\\d+", "m\\d+", "m.*[05]|u400|pd"]
UNION_EXPECTED = {p: ref.assert_selective(UDOCS, p) for p in UNION_PATTERNS}
assert len(ref.matched_terms("m\\d+", ref.term_set(UDOCS))) > 4096
assert len(ref.matched_terms("c\\d+", ref.term_set(UDOCS))) > 100
for _d in (0, 31, 32, TILE_DOCS - 1, TILE_DOCS, UN - 1):
    assert _d in UNION_EXPECTED["p[a-f]"]
assert UN % 32 != 0


@pytest.fixture(scope="module")
def gpu():
    import __graft_entry__
    __graft_entry__.build()
    from quickwit_amd.api import GpuSearcher
    g = GpuSearcher(device=0)
    for n, docs in DICT_DOCS.items():
        g.add_split("d%d" % n, make_split(docs, "d%d" % n))
    g.add_split("un", make_split(UDOCS, "un"))
    return g


# ---------------------------------------------------------- dictionary scan
@pytest.mark.parametrize("n_terms", DICT_SIZES)
def test_dictionary_scan_edges(gpu, n_terms):
    docs = DICT_DOCS[n_terms]
    before = launches(gpu, "k_dict_dfa_match")
    for (n, p), exp in DICT_EXPECTED.items():
        if n == n_terms:
            check(gpu, regex(p), "d%d" % n, len(docs), exp)
    assert launches(gpu, "k_dict_dfa_match") > before


def test_raw_field_long_term_and_no_auto_case_fold(gpu):
    long_tag = "A" * 200
    tags = [long_tag, "Tag-One", "Tag-Two", "other", "Tag-One"]
    w = splitgen.SplitWriter(SCHEMA, "raw", store_docs=False)
    w.add_documents([{"tag": t, "body": "zz", "n": 1, "k": "k"} for t in tags])
    gpu.add_split("raw", w.finalize())
    check(gpu, regex("A{200}", "tag"), "raw", 5, [0])
    check(gpu, regex("A{199}", "tag"), "raw", 5, [])
    check(gpu, regex("Tag-.*", "tag"), "raw", 5, [1, 2, 4])
    # a raw tokenizer does not lowercase: no "(?i)" is added
    check(gpu, regex("tag-.*", "tag"), "raw", 5, [])
    check(gpu, regex("(?i)tag-o.*", "tag"), "raw", 5, [1, 4])
    # the default tokenizer lowercases: "(?i)" is added
    check(gpu, regex("ZZ"), "raw", 5, [0, 1, 2, 3, 4])


# -------------------------------------------------------------------- union
@pytest.mark.parametrize("pattern", UNION_PATTERNS)
def test_union_edges(gpu, pattern):
    before = launches(gpu, "k_terms_union_bitmap")
    check(gpu, regex(pattern), "un", UN, UNION_EXPECTED[pattern])
    assert launches(gpu, "k_terms_union_bitmap") == before + 1


def test_no_matching_term(gpu):
    assert not ref.matched_terms("nomatch.*", ref.term_set(UDOCS))
    before = launches(gpu, "k_terms_union_bitmap")
    scans = launches(gpu, "k_dict_dfa_match")
    check(gpu, regex("nomatch.*"), "un", UN, [])
    check(gpu, {"type": "bool", "must": [regex("nomatch.*"), term("zz")]},
          "un", UN, [])
    assert launches(gpu, "k_dict_dfa_match") > scans
    assert launches(gpu, "k_terms_union_bitmap") == before


# -------------------------------------------------------------- composition
def docs_with(t):
    return {d for d, toks in enumerate(UDOCS) if t in toks}


def test_inside_bool(gpu):
    u = set(UNION_EXPECTED["u.*"])
    m = set(UNION_EXPECTED["m\\d+"])
    u400 = docs_with("u400")
    assert u & m and m - u400 and u400 - m
    check(gpu, {"type": "bool", "must": [regex("m\\d+"), term("u400")]},
          "un", UN, sorted(m & u400))
    check(gpu, {"type": "bool", "filter": [regex("m\\d+")],
                "must": [term("u400")]}, "un", UN, sorted(m & u400))
    check(gpu, {"type": "bool", "must": [term("u400")],
                "must_not": [regex("m\\d+")]}, "un", UN, sorted(u400 - m))
    check(gpu, {"type": "bool", "should": [regex("u12[789]"), term("pa")]},
          "un", UN, sorted(set(UNION_EXPECTED["u12[789]"]) | {0}))
    check(gpu, {"type": "bool", "must": [regex("u.*"), regex("m\\d+")]},
          "un", UN, sorted(u & m))


def test_count_only(gpu):
    r = search(gpu, regex("m\\d+"), [("un", UN)], max_hits=0)
    assert not r.get("failed_splits")
    assert r["num_hits"] == len(UNION_EXPECTED["m\\d+"])
    assert not r.get("partial_hits")


def test_with_terms_agg_and_fast_field_sort(gpu):
    """The same doc set through an OR of the three terms the regex matches:
    aggregation and sorted hits must be identical."""
    same = {"type": "bool", "should": [term("u127"), term("u128"),
                                       term("u129")]}
    aggs = {"by_k": {"terms": {"field": "k"}}}
    sort = [{"field_name": "n", "sort_order": 1}]
    out = []
    for q in (regex("u12[789]"), same):
        r = search(gpu, q, [("un", UN)], max_hits=50, aggregation=aggs,
                   sort_fields=sort)
        assert not r.get("failed_splits"), r.get("failed_splits")
        agg = gpu.finalize_agg_json(r["intermediate_aggregation_result"], aggs)
        out.append((r["num_hits"], [(h.get("doc_id", 0), h.get("sort_value"))
                                    for h in r["partial_hits"]], agg))
    assert out[0] == out[1]
    assert out[0][0] == len(UNION_EXPECTED["u12[789]"])
    counts = {b["key"]: b["doc_count"] for b in out[0][2]["by_k"]["buckets"]}
    exp = {}
    for d in UNION_EXPECTED["u12[789]"]:
        exp["k%d" % (d % 3)] = exp.get("k%d" % (d % 3), 0) + 1
    assert counts == exp


def test_two_segment_split(gpu):
    a, b = UDOCS[:5000], UDOCS[5000:]
    data = splitgen.concat_segments(
        [make_split(a, "ms"), make_split(b, "ms")], "ms")
    gpu.add_split("ms", data)
    for p in ("u.*", "m.*[05]|u400|pd"):
        r = search(gpu, regex(p), [("ms", UN)], max_hits=UN)
        assert not r.get("failed_splits"), r.get("failed_splits")
        got = sorted((h.get("segment_ord", 0), h.get("doc_id", 0))
                     for h in r.get("partial_hits", []))
        exp = [(0, d) for d in ref.regex_hits(a, p)] + \
              [(1, d) for d in ref.regex_hits(b, p)]
        assert exp and got == exp, p


def test_second_run_served_from_hitset_cache(gpu):
    q = regex("u40+|c1\\d\\d")
    exp = ref.assert_selective(UDOCS, "u40+|c1\\d\\d")
    check(gpu, q, "un", UN, exp)
    scans = launches(gpu, "k_dict_dfa_match")
    unions = launches(gpu, "k_terms_union_bitmap")
    check(gpu, q, "un", UN, exp)
    assert launches(gpu, "k_dict_dfa_match") == scans
    assert launches(gpu, "k_terms_union_bitmap") == unions


# ------------------------------------------------------------------ surface
def error_of(gpu, query, **kw):
    """The error text of a refused query: a failed call or failed splits."""
    try:
        r = search(gpu, query, [("un", UN)], **kw)
    except RuntimeError as e:
        return str(e)
    assert r.get("failed_splits") and r.get("num_hits", 0) == 0, query
    return r["failed_splits"][0]["error"]


def test_refusals_are_errors(gpu):
    score = [{"field_name": "_score", "sort_order": 1}]
    assert "const-score" in error_of(gpu, regex("u.*"), max_hits=5,
                                     sort_fields=score)
    assert "non-text field" in error_of(gpu, regex("1", "n"))
    assert "unknown field" in error_of(gpu, regex("a", "nope"))
    msg = error_of(gpu, regex("red$"))
    assert "invalid regex" in msg and "$" in msg
    assert "multiple fields" in error_of(
        gpu, {"type": "user_input", "user_text": "/u.*/",
              "default_fields": ["body", "tag"]})
    # the searcher still answers afterwards
    check(gpu, regex("u1"), "un", UN, UNION_EXPECTED["u1"])


def test_grammar_literal(gpu):
    for text, dfs in (("body:/u12[789]/", []), ("/u12[789]/", ["body"]),
                      ("body:/U12[789]/", [])):
        q = {"type": "user_input", "user_text": text, "default_fields": dfs}
        check(gpu, q, "un", UN, UNION_EXPECTED["u12[789]"])
    q = {"type": "user_input", "user_text": "body:/m\\d+/ AND body:u400",
         "default_fields": []}
    check(gpu, q, "un", UN,
          sorted(set(UNION_EXPECTED["m\\d+"]) & docs_with("u400")))


# ------------------------------------------------------------------ goldens
@pytest.fixture(scope="module")
def es_client():
    from fastapi.testclient import TestClient

    from quickwit_amd.api import GpuSearcher
    from quickwit_amd.rest import create_app
    return TestClient(create_app(lambda: GpuSearcher(device=0)))


def golden(name):
    with open(os.path.join(REPO, "tests", "golden", name)) as f:
        return json.load(f)


def test_regex_scenarios_replay(es_client):
    from rest_replay import run_step
    suite = golden("rest_scenarios.json")["suites"]["es_compatibility"]
    first_search = next(i for i, s in enumerate(suite)
                        if s["endpoint"].endswith("_search"))
    for step in suite[:first_search]:  # index creation + ingest
        run_step(es_client, step)
    steps = golden("regex_scenarios.json")["steps"]
    assert len(steps) == 7
    ours = [s for s in steps if "elasticsearch" not in s.get("engines", [])]
    assert len(ours) == 5
    for step in ours:
        run_step(es_client, step)
    # type:/pushevent/ through query_string
    assert ours[-1]["json"]["query"]["query_string"]["query"] == \
        "type:/pushevent/"
    assert ours[-1]["expected"]["hits"]["total"]["value"] == 60


def test_es_compat_extra_without_regexp_skip(es_client):
    from rest_replay import replay_suite

    def skip_only_stats(i, step):
        if step.get("endpoint") == "_stats":
            return "global _stats totals depend on cross-suite session state"
        return None

    steps = golden("rest_scenarios.json")["suites"]["es_compat_extra"]
    jour = [s for s in steps if "regexp" in json.dumps(s.get("json", {}))]
    assert len(jour) == 1
    assert jour[0]["expected"]["hits"]["total"]["value"] == 3
    ran, skipped = replay_suite(es_client, steps, skip_only_stats)
    assert ran >= 130 and len(skipped) == 1, (ran, skipped)
