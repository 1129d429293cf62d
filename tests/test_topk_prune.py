"""Top-K pruning in the leaf tile kernel, against the exact
float64 reference of tests/topk_reference.py.

Every case runs on two searchers in one process: the default config (pruning
on where the gate allows) and {"topk_prune": False}. Both must return what
ref.expected says: ids, num_hits and values exactly, scores at ref.REL.
GpuSearcher.topk_stats() tells a working prune from one that is silently off.

The gate (product.cpp): collecting call, narrow 8-byte records (one-field
_score sort or doc order), no search_after, 1 <= K <= 64 with K = max_hits +
start_offset, and the context has not disabled it.

Which path the other files reach now: the narrow K <= 64 cases of
tests/test_topk_exact.py (K = 1 and 10 of the tied and class corpora, K = 10
of the order-dependent ones, small edge-sweep splits) run pruned; its
K >= 4096, wide-record and search_after cases are outside the gate and keep
exercising the histogram refinement exactly as before.

Emitted-count cap on the tied corpus: all 70,000 docs share one score, so the
key is monotone in doc id and a tile's own bound lets through at most the K
highest words of its best wave, 32 docs each: emitted <= 32 * K * n_tiles.
(The ninth tile is partial; when its best wave has fewer than K words the
bound comes from the wave below and that tile alone can exceed 32 * K by up
to 368 docs. The total then passes the cap only if every one of the eight
full tiles also read a stale bound, i.e. they finished in ascending order
and all before the half-sized tile.)
"""
import numpy as np
import pytest

import topk_reference as ref
from quickwit_amd.api import GpuSearcher, make_leaf_request

pytestmark = pytest.mark.gpu

TILE = 8192
WAVE_SPAN = 2048  # docs per wave of a tile: 64 words x 32 docs


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


class Pair:
    """A pruned and an unpruned device context over the same splits."""

    def __init__(self):
        self.on = GpuSearcher(device=0)
        self.off = GpuSearcher(device=0, config={"topk_prune": False})
        self.loaded = set()

    def run(self, c, q, sort, max_hits, start_offset=0):
        """{"on"/"off": (hits, stats delta, last emitted, last matched)}"""
        if c.split_id not in self.loaded:
            for s in (self.on, self.off):
                s.add_split(c.split_id, c.data)
            self.loaded.add(c.split_id)
        req = make_leaf_request(
            q.ast(), ref.SCHEMA, [(c.split_id, c.num_docs)], max_hits=max_hits,
            start_offset=start_offset,
            sort_fields=ref.sort_fields(sort) or None)
        out = {}
        for tag, s in (("on", self.on), ("off", self.off)):
            before = s.topk_stats()
            try:
                resp = s.leaf_search(req)
            except RuntimeError as e:
                # a device error is not a mismatch: start nothing more
                pytest.exit(f"leaf_search failed, stopping the run: {e}", 3)
            after = s.topk_stats()
            out[tag] = (ref.hits_of(resp), after[0] - before[0],
                        after[1] - before[1], after[2], after[3])
        return out


@pytest.fixture(scope="module")
def pair():
    return Pair()


def check_both(pair, c, q, sort, k, start_offset=0, what=""):
    """Both searchers equal the reference; returns the run record."""
    exp = ref.expected(c, q, sort, k, start_offset)
    out = pair.run(c, q, sort, k, start_offset)
    for tag in ("on", "off"):
        ref.assert_hits_exact(out[tag][0], exp, sort, (what, tag))
    # the unpruned context never prunes
    assert out["off"][1] == 0
    return out


def gate_open(sort, k_total):
    narrow = len(sort) == 0 or (len(sort) == 1 and sort[0][0] == "_score")
    return narrow and 1 <= k_total <= 64


# ------------------------------------------------------------- tied corpus
TIED = [(sort, k, 0) for sort in (ref.SCORE_DESC, ref.SCORE_ASC)
        for k in (1, 10, 63, 64, 65)] + \
       [(sort, 10, off) for sort in (ref.SCORE_DESC, ref.SCORE_ASC)
        for off in (54, 60)]


@pytest.mark.parametrize(
    "sort,k,off", TIED,
    ids=[f"{'desc' if s[0][1] else 'asc'}-k{k}-off{o}" for s, k, o in TIED])
def test_tied(pair, sort, k, off):
    c = ref.tied_corpus()
    out = check_both(pair, c, ref.AA, sort, k, off, "tied")
    K = k + off
    n_tiles = -(-c.num_docs // TILE)
    _, pruned, unpruned, emitted, matched = out["on"]
    assert matched == c.num_docs
    if K <= 64:
        assert (pruned, unpruned) == (1, 0)
        print(f"tied K={K}: emitted {emitted} of {matched}")
        assert K <= emitted <= 32 * K * n_tiles
    else:
        assert (pruned, unpruned) == (0, 1)
        assert emitted == matched
    _, pruned, unpruned, emitted, matched = out["off"]
    assert (pruned, unpruned) == (0, 1)
    assert emitted == matched == c.num_docs


# -------------------------------------------------------------- edge sweep
@pytest.mark.parametrize("n", ref.EDGE_SIZES)
def test_edge_sweep(pair, n):
    """n < K (the bound must stay 0), 1-doc splits, partial last tiles, the
    8192 / 16384 tile edges."""
    c = ref.edge_corpus(n)
    for name, q, sort, k0 in ref.edge_queries(n):
        for k in ((1, 10, 64) if k0 else (0,)):
            out = check_both(pair, c, q, sort, k, what=(n, name, k))
            _, pruned, unpruned, emitted, matched = out["on"]
            if k == 0:
                assert (pruned, unpruned) == (0, 0)  # count-only: no collect
                continue
            assert pruned + unpruned <= 1  # 0: hits enumerable without kernel
            if pruned + unpruned:
                assert pruned == int(gate_open(sort, k))
                assert min(k, matched) <= emitted <= matched
                if matched <= k or not pruned:
                    assert emitted == matched
            if out["off"][1] + out["off"][2]:
                assert out["off"][3] == out["off"][4]


# --------------------------------------------------------------- placement
N_PLACE = 20_000  # three tiles: 8192 + 8192 + 3616
K_PLACE = 10


def _place_columns(n):
    d = np.arange(n)
    present = np.ones(n, dtype=bool)
    return {"u": ((d % 5).astype(np.uint64), present),
            "i": (d.astype(np.int64), present),
            "f": (d * 0.5, present)}


def _placement_corpus(name):
    """'aa' with tf 1 on the background matches and tf 5 on the K best."""
    n, k = N_PLACE, K_PLACE
    rng = np.random.default_rng(31)
    tf = np.zeros(n, dtype=np.int64)
    if name in ("first-tile", "last-tile"):
        # ~25% background density everywhere; the best K inside one tile
        tf[ref.scatter(n, [n // 4, 0], seed=7) == 0] = 1
        lo, hi = (0, TILE) if name == "first-tile" else (2 * TILE, n)
        tf[rng.choice(np.arange(lo, hi), k, replace=False)] = 5
    elif name == "one-per-wave":
        # ten 2048-doc wave spans (the last one partial), one best doc in
        # each; the background fills 5 whole words per span, so no wave has
        # K non-empty words and every tile's bound is 0
        for w in range(k):
            lo = w * WAVE_SPAN
            words = rng.choice((min(n, lo + WAVE_SPAN) - lo) // 32 - 1, 5,
                               replace=False)
            for wd in words:
                tf[lo + wd * 32: lo + wd * 32 + 32] = 1
            tf[lo + words[0] * 32 + int(rng.integers(0, 32))] = 5
    elif name == "few-matches":
        tf[rng.choice(n, k - 3, replace=False)] = rng.integers(1, 6, k - 3)
    else:
        raise AssertionError(name)
    return ref.Corpus(f"prune-{name}", {"aa": tf}, np.full(n, 16),
                      _place_columns(n))


PLACEMENTS = ("first-tile", "last-tile", "one-per-wave", "few-matches")


@pytest.mark.parametrize("name", PLACEMENTS)
@pytest.mark.parametrize("sort", [ref.SCORE_DESC, ref.SCORE_ASC],
                         ids=["desc", "asc"])
def test_placement(pair, name, sort):
    c = _placement_corpus(name)
    out = check_both(pair, c, ref.AA, sort, K_PLACE, what=name)
    _, pruned, unpruned, emitted, matched = out["on"]
    assert (pruned, unpruned) == (1, 0)
    assert min(K_PLACE, matched) <= emitted <= matched
    if sort == ref.SCORE_DESC and name in ("first-tile", "last-tile"):
        # the K best carry tf 5; the reference must agree they are the hits
        got_ids = {d for d, _, _ in out["on"][0][1]}
        assert got_ids == set(np.nonzero(c.tf("aa") == 5)[0].tolist())
    if name in ("one-per-wave", "few-matches"):
        assert emitted == matched  # bound stayed 0: nothing pruned
    else:
        # ~5,000 background matches at 25% density: every wave of every tile
        # has K non-empty words, so each tile's own bound is above the keys
        # of its worst wave and something is dropped in any tile order
        assert emitted < matched
    assert out["off"][3] == out["off"][4] == matched


# ------------------------------------------------- order-dependent (flagship)
def order_dependent_properties(c, q, sort, k, num_hits, hits):
    """The property checks of test_topk_exact.test_order_dependent: f32 sums
    of three terms depend on arrival order, so list equality is not fixed;
    everything below is."""
    desc = sort[0][1] == ref.DESC
    n, full = ref.ranked(c, q, sort)
    assert num_hits == n
    assert len(hits) == min(k, n)
    s64 = ref.scores64(c, q)
    ids = [d for d, _, _ in hits]
    assert len(set(ids)) == len(ids)
    for d, s, _ in hits:
        assert abs(s - s64[d]) / s64[d] <= ref.REL, (d, s, s64[d])
    for (da, sa, _), (db, sb, _) in zip(hits, hits[1:]):
        before = (sa, da) > (sb, db) if desc else (sa, da) < (sb, db)
        assert before, ((da, sa), (db, sb))
    want_share, members = {}, {}
    for rank, (d, s, _) in enumerate(full):
        members.setdefault(s, set()).add(d)
        if rank < k:
            want_share[s] = want_share.get(s, 0) + 1
    got_by_class = {}
    for d in ids:
        got_by_class.setdefault(float(s64[d]), set()).add(d)
    assert set(got_by_class) == set(want_share)
    for s, share in want_share.items():
        if share == len(members[s]):
            assert got_by_class[s] == members[s], ("class", s)
        else:
            assert len(got_by_class[s]) == share, ("cut class", s)
    left = np.ones(c.num_docs, dtype=bool)
    left[ids] = False
    left &= ref.match_mask(c, q)
    last = hits[-1][1]
    if desc:
        assert not (s64[left] * (1 - ref.REL) > last).any()
    else:
        assert not (s64[left] * (1 + ref.REL) < last).any()


@pytest.mark.parametrize("sort", [ref.SCORE_DESC, ref.SCORE_ASC],
                         ids=["desc", "asc"])
def test_order_dependent_shape(pair, sort):
    """The flagship's shape: a 3-term disjunction by _score at K = 10."""
    c = ref.classes_corpus()
    name, q = ref.ORDER_DEPENDENT[0]
    assert len(q.scoring_terms) == 3
    out = pair.run(c, q, sort, 10)
    for tag in ("on", "off"):
        num_hits, hits = out[tag][0]
        order_dependent_properties(c, q, sort, 10, num_hits, hits)
    assert (out["on"][1], out["on"][2]) == (1, 0)
    assert (out["off"][1], out["off"][2]) == (0, 1)
    assert 10 <= out["on"][3] <= out["on"][4]
    assert out["off"][3] == out["off"][4]
