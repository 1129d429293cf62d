"""Float64 reference for scored boolean TREES, and the corpus and cases of
the gated-BM25 tests.

Plain helper module (not a conftest): numpy and topk_reference.Corpus only —
nothing from the oracle or the product. test_score_tree_cpu.py proves it
against the oracle on a machine without a GPU; test_score_tree_gpu.py then
holds the HIP path to it.

Semantics (oracle.cpp eval / eval_bool, restated over the token matrix):
  match(node, d)   the unscored boolean semantics: must and filter children
                   all match, no must_not child matches, and at least
                   minimum_should_match should children match (unset: 1
                   without a must/filter child, else 0; without one, a doc
                   must still occur in some should child)
  score(term, d)   W * tf / (tf + K_d), W = idf * (1 + k1) * boost
  score(other leaf) 0: range and match_all leaves match, never score
  score(bool, d)   boost * sum of score(c, d) over its must and should
                   children c with match(c, d); 0 where the bool itself does
                   not match; filter and must_not children never score

Queries are the engine's own query-AST dicts (bool / term / range / boost /
match_all), so the same object goes to the engines and to evaluate().

Comparison rule (compare): scores pointwise within REL; doc ids equal as
sets within each group of equal reference key, except the group the end of
the page cuts, whose returned ids must belong to it. An f32 sum of three or
more contributions depends on arrival order in its last bit (see the note at
the top of topk_reference.py), so inside a group the order is not pinned.
The rule is sound only if distinct reference scores are further apart than
the tolerance: min_score_gap() measures that, the CPU test asserts it.
"""
import functools
import math

import numpy as np

import topk_reference as tr
from topk_reference import Corpus

FIELD = tr.FIELD
K1, B = tr.K1, tr.B
REL = tr.REL
ASC, DESC = tr.ASC, tr.DESC
SCHEMA = tr.SCHEMA
SCORE_DESC, SCORE_ASC = [("_score", DESC)], [("_score", ASC)]
GAP = 1e-4  # distinct reference scores differ by more than this, relative


# ------------------------------------------------------------ query AST
def term(w):
    return {"type": "term", "field": FIELD, "value": w}


def rng(col, lo, hi):
    return {"type": "range", "field": col, "lower_bound": {"included": lo},
            "upper_bound": {"included": hi}}


def boost(b, node):
    return {"type": "boost", "underlying": node, "boost": b}


def bool_(must=(), should=(), filter=(), must_not=(), msm=None):
    q = {"type": "bool"}
    for key, clauses in (("must", must), ("should", should),
                         ("filter", filter), ("must_not", must_not)):
        if clauses:
            q[key] = [term(c) if isinstance(c, str) else c for c in clauses]
    if msm is not None:
        q["minimum_should_match"] = msm
    return q


# ------------------------------------------------------------- evaluator
def _kd(c):
    lengths = c.lengths
    avgdl = float(lengths.sum()) / c.num_docs
    return K1 * (1.0 - B + B * tr.quantize_lengths(lengths).astype(np.float64)
                 / (avgdl if avgdl > 0 else 1.0))


def evaluate(c, node):
    """(match bool[N], score float64[N]); score is 0 where match is False."""
    n = c.num_docs
    zero = np.zeros(n, dtype=np.float64)
    t = node["type"]
    if t == "match_all":
        return np.ones(n, dtype=bool), zero
    if t == "boost":
        m, s = evaluate(c, node["underlying"])
        return m, s * float(node["boost"])
    if t == "term":
        assert node["field"] == FIELD
        tf = c.tf(node["value"]).astype(np.float64)
        m = tf > 0
        df = int(m.sum())
        if df == 0:
            return m, zero
        idf = math.log(1.0 + (n - df + 0.5) / (df + 0.5))
        return m, (idf * (1.0 + K1)) * tf / (tf + _kd(c))
    if t == "range":
        vals, present = c.columns[node["field"]]
        lo = node["lower_bound"]["included"]
        hi = node["upper_bound"]["included"]
        return present & (vals >= lo) & (vals <= hi), zero
    assert t == "bool", t
    must = [evaluate(c, x) for x in node.get("must", [])]
    filt = [evaluate(c, x) for x in node.get("filter", [])]
    should = [evaluate(c, x) for x in node.get("should", [])]
    must_not = [evaluate(c, x) for x in node.get("must_not", [])]
    msm = node.get("minimum_should_match")
    if not (must or filt or should or must_not) and (msm is None or msm <= 0):
        return np.ones(n, dtype=bool), zero  # empty bool = match_all
    m = np.ones(n, dtype=bool)
    for cm, _ in must + filt:
        m &= cm
    cnt = np.zeros(n, dtype=np.int64)
    for cm, _ in should:
        cnt += cm
    if must or filt:
        need = 0 if msm is None or msm < 0 else msm
        if should and need > 0:
            m &= cnt >= need
    elif should:
        need = 1 if msm is None or msm < 0 else msm
        m &= cnt >= max(need, 1)
    elif not must_not:
        m[:] = False
    for cm, _ in must_not:
        m &= ~cm
    s = zero.copy()
    for _, cs in must + should:
        s += cs  # a child's score is already 0 where the child does not match
    return m, np.where(m, s, 0.0)


def _f64_sortable(v):
    bits = np.asarray(v, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | tr.SIGN)


def ranked(c, node, sort=SCORE_DESC):
    """(num_hits, [(doc, score64, key), ...]) of EVERY matching doc in sort
    order (sorting.md: each value in its order, a missing value last, then
    doc id in the primary direction). key identifies the hit's tie group:
    the tuple of its sort values. sort: one or two (field, order) entries of
    "_score" or the "u" column. Cached per corpus."""
    import json
    ck = ("tree", json.dumps(node, sort_keys=True), tuple(sort))
    if ck in c._cache:
        return c._cache[ck]
    m, s = evaluate(c, node)
    docs = np.nonzero(m)[0]
    d64 = docs.astype(np.uint64)
    keys = [d64 if sort[0][1] == ASC else ~d64]  # least significant first
    group = []
    for field, order in reversed(sort):
        if field == "_score":
            key, present, vals = _f64_sortable(s), np.ones(len(s), bool), s
        else:
            vals, present = c.columns[field]
            key = vals
        key, present = key[docs], present[docs]
        key = np.where(present, key if order == ASC else ~key, np.uint64(0))
        keys += [key, ~present]
        group.insert(0, (vals[docs], present))
    perm = np.lexsort(keys)
    gcols = [[v if p else None for v, p in zip(vals[perm].tolist(),
                                                present[perm].tolist())]
             for vals, present in group]
    out = (len(docs), list(zip(docs[perm].tolist(), s[docs][perm].tolist(),
                               zip(*gcols))))
    c._cache[ck] = out
    return out


def min_score_gap(c, node):
    """Smallest relative distance between two distinct scores of matches."""
    m, s = evaluate(c, node)
    vals = np.unique(s[m])
    vals = vals[vals > 0]
    if len(vals) < 2:
        return math.inf
    return float(((vals[1:] - vals[:-1]) / vals[1:]).min())


# ------------------------------------------------------------- comparison
def hits_of(resp):
    """[(doc_id, score)] of a LeafSearchResponse dict; the score is whichever
    sort value carries an f64 (the columns used here are u64)."""
    out = []
    for h in resp.get("partial_hits", []):
        sc = None
        for k in ("sort_value", "sort_value2"):
            if "f64" in (h.get(k) or {}):
                sc = h[k]["f64"]
        out.append((h.get("doc_id", 0), sc))
    return out


def compare(got, full, start, page, what=""):
    """got: [(doc, score)] as returned; full: ranked()[1]; the page is
    full[start:start + page]. Applies the module's comparison rule and
    returns the largest relative score deviation seen."""
    exp = full[start:start + page]
    assert len(got) == len(exp), (what, "hit count", len(got), len(exp))
    worst = 0.0
    for r, ((_, gs), (_, es, _)) in enumerate(zip(got, exp)):
        assert gs is not None, (what, "no score", r)
        assert math.isclose(gs, es, rel_tol=REL, abs_tol=0.0), \
            (what, "score", r, gs, es)
        if es:
            worst = max(worst, abs(gs - es) / es)
    end = start + len(exp)
    i = 0
    while i < len(exp):
        j = i
        while j < len(exp) and exp[j][2] == exp[i][2]:
            j += 1
        ids = {d for d, _ in got[i:j]}
        assert len(ids) == j - i, (what, "duplicate ids", i)
        cut = j == len(exp) and end < len(full) and full[end][2] == exp[i][2]
        if cut:
            k = end
            while k < len(full) and full[k][2] == exp[i][2]:
                k += 1
            allowed = {d for d, _, _ in full[start + i:k]}
            assert ids <= allowed, (what, "cut group", i, sorted(ids - allowed))
        else:
            want = {d for d, _, _ in exp[i:j]}
            assert ids == want, (what, "group", i, sorted(ids ^ want)[:10])
        i = j
    return worst


# ----------------------------------------------------------------- corpus
TILE_DOCS = 8192  # gpu_types.h
N_DOCS = 2 * TILE_DOCS + 37  # three tiles, the last one partial
ABSENT = "nope"  # not in the dictionary

WORDS = ("a", "b", "c", "d", "x", "m")
# 'a' is dense (df near N/2: consecutive 128-posting blocks straddle both
# tile edges); 'x' has one short block; 'm' is cleared from the middle tile
# below. The five-doc (0,0,6,6) class scores highest under the OR-of-ANDs
# query with a TWO-term sum, which is exact: a cursor inside it is stable.
CLASS_TABLE = [
    (3_000, (1, 0, 0, 0, 0, 0)),
    (2_500, (2, 1, 0, 0, 0, 0)),
    (2_000, (1, 2, 1, 0, 0, 0)),
    (1_500, (0, 1, 2, 0, 0, 1)),
    (1_500, (0, 0, 1, 2, 0, 0)),
    (1_200, (3, 0, 3, 1, 0, 2)),
    (1_000, (0, 3, 0, 1, 0, 0)),
    (800,   (0, 0, 0, 3, 0, 1)),
    (40,    (1, 1, 1, 0, 1, 0)),
    (600,   (1, 1, 1, 1, 0, 0)),
    (5,     (0, 0, 6, 6, 0, 0)),
    (0,     (0, 0, 0, 0, 0, 0)),  # the rest: 2,276
]


def _build(split_id, n, seed):
    # the table is sized for N_DOCS; a smaller corpus scales the big classes
    cls = tr.scatter(n, [cnt if cnt <= 40 else cnt * n // N_DOCS
                         for cnt, _ in CLASS_TABLE], seed)
    tfs = np.array([t for _, t in CLASS_TABLE], dtype=np.int64)
    tf = {w: tfs[cls, j].copy() for j, w in enumerate(WORDS)}
    d = np.arange(n)
    tf["m"][(d >= TILE_DOCS) & (d < 2 * TILE_DOCS)] = 0
    u = tr.column_from_groups(n, "u", [(1, n // 4), (2, n // 4), (3, n // 4),
                                       (None, 0)], seed + 1)
    cols = {"u": u, "i": (d.astype(np.int64) - 100, np.ones(n, bool)),
            "f": (d * 0.5, np.ones(n, bool))}
    return Corpus(split_id, tf, np.full(n, 16), cols)


@functools.lru_cache(maxsize=None)
def corpus():
    return _build("score-tree", N_DOCS, seed=17)


@functools.lru_cache(maxsize=None)
def second_segment():
    """A smaller second segment for the two-segment split (one tile + 1)."""
    return _build("score-tree-seg1", TILE_DOCS + 1, seed=29)


# ------------------------------------------------------------------ cases
OR_OF_ANDS = bool_(should=[bool_(must=["a", "b"]), bool_(must=["c", "d"])])

# every case is refused by a product that only flattens (failed split)
CASES = [
    ("core-gate", bool_(must=["a"], should=[bool_(must=["b", "c"])])),
    ("or-of-ands", OR_OF_ANDS),
    ("must_not-in-gated", bool_(should=["x", bool_(must=["c"],
                                                   must_not=["d"])])),
    ("depth3-two-gates", bool_(should=[bool_(
        must=["a"], should=[bool_(must=["b", "c"])])])),
    ("boosts", boost(1.5, bool_(must=["a"], should=[boost(2.0, bool_(
        must=[boost(0.5, term("b")), "c"]))]))),
    ("filter-nested", bool_(must=["a"], filter=[bool_(must=["b"],
                                                      must_not=["d"])])),
    ("msm2-of-3", bool_(should=["b", "c", "d"], msm=2)),
    ("msm1-with-must", bool_(must=["a"], should=["b", "m"], msm=1)),
    ("range-should", bool_(should=["x", rng("u", 1, 2)])),
    ("repeated-term", bool_(should=[bool_(must=["b", "c"]),
                                    bool_(must=["b", "d"])])),
    ("empty-nested", bool_(should=["a", bool_(must=[ABSENT, "b"])])),
    ("absent-middle-gated", bool_(should=["x", bool_(must=["m", "d"])])),
]
