"""One-sync top-K selection, against the exact float64
reference of tests/topk_reference.py.

A collecting call without a search_after cursor lets the device pick the
K-boundary bin of the pass-0 histogram and compact the survivors behind the
tile kernel (k_cand_pick_compact); the first S = TOPK_INLINE_SURVIVORS survivor
records come down with the call's one synchronize, a longer list costs one
more copy of its tail, and a boundary bin of more than
T = max(4 K, 16384) records sets a flag that sends select() into its host
refinement loop (the fallback).

Every GPU case runs on two contexts in one process: the default one and
{"topk_onesync": False}. Both must return what ref.expected says under
ref.assert_hits_exact. GpuSearcher.topk_onesync_stats() tells which path ran,
so a silently disabled fast path fails here; the second context must never
move its counters.

Which path a case takes is worked out on the CPU first (pick_model below, the
host loop's first iteration in numpy over the reference's keys; test_model_*
pin the table without a GPU) and then demanded of the device:

  narrow key   f32-sortable score << 32 | doc, both halves complemented when
               ascending; doc order carries no score, so all its keys share
               bin 0 (4095 ascending)
  pass-0 bin   the key's top 12 bits: sign, exponent, 3 mantissa bits
  pruned       the tile kernel emits at most the docs of each tile's K best
               32-doc words (test_topk_prune.py): <= 32 K n_tiles = 2,880
               records at K = 10 over nine tiles, below T, so every emitted
               record survives and the survivor count is the emitted count
  unpruned     all 70,000 matches are candidates; the model says how many
               share the boundary bin

The model rounds the float64 reference score to f32 where the device sums in
f32; the two can differ in the last bit, which moves a doc across a bin edge
only if a score class sits within one ulp of a multiple of 2^20 ulps. The
one- and two-term classes used here do not (test_model_classes_unpruned pins
their counts; the device must report the same).
"""
import numpy as np
import pytest

import topk_reference as ref
from quickwit_amd.api import GpuSearcher, make_leaf_request

S = 4096          # TOPK_INLINE_SURVIVORS (gpu_types.h); test_sizes pins it
T_MIN = 16384     # TOPK_REFINE_MIN
BINS = 4096
ALL = ref.Query(should=["all"])  # every doc of an edge corpus, one score


# ------------------------------------------------------------------ model
def _f32_sortable(s):
    b = np.asarray(s, dtype=np.float32).view(np.uint32)
    return np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(1 << 31))


def narrow_keys(c, q, sort):
    """Device keys of every match under a narrow sort (_score or doc order)."""
    m = ref.match_mask(c, q)
    docs = np.nonzero(m)[0].astype(np.uint64)
    if sort:
        kh = _f32_sortable(ref.scores64(c, q)[m]).astype(np.uint64)
    else:
        kh = np.zeros(len(docs), dtype=np.uint64)
    keys = (kh << np.uint64(32)) | docs
    return ~keys if sort and sort[0][1] == ref.ASC else keys


def wide_u_keys(c, q, order):
    """Selection keys of a sort by the u64 column: the value (complemented
    when ascending), 0 for a missing one."""
    m = ref.match_mask(c, q)
    vals, present = c.columns["u"]
    keys = vals[m] if order == ref.DESC else ~vals[m]
    return np.where(present[m], keys, np.uint64(0))


def pick_model(keys, kwant):
    """(survivors, fallback) of the device pick over all `keys`."""
    n = len(keys)
    k = min(kwant, n)
    t = max(4 * k, T_MIN)
    if n <= t:
        return n, False
    hist = np.bincount((keys >> np.uint64(52)).astype(np.int64), minlength=BINS)
    cum = 0
    b = BINS - 1
    while b > 0 and cum + hist[b] < k:
        cum += hist[b]
        b -= 1
    survivors = int(cum + hist[b])
    return survivors, survivors > t


NARROW_SORTS = [("desc", ref.SCORE_DESC), ("asc", ref.SCORE_ASC), ("doc", [])]
NARROW = [(qn, q, sn, sort, k)
          for qn, q in (("aa", ref.AA), ("bbcc", ref.BB_CC))
          for sn, sort in NARROW_SORTS for k in (1, 10)]
NARROW_IDS = [f"{qn}-{sn}-k{k}" for qn, _, sn, _, k in NARROW]

# what pick_model says of the unpruned narrow cases on classes_corpus:
# (survivors, fallback). Doc order puts every key into one bin.
UNPRUNED_PATHS = {
    # 'aa': tf classes of 3 / 17,000 / 100 / 30,000 / 22,897 docs, best first
    "aa-desc-k1": (3, False), "aa-desc-k10": (17_003, True),
    "aa-asc-k1": (22_897, True), "aa-asc-k10": (22_897, True),
    "aa-doc-k1": (70_000, True), "aa-doc-k10": (70_000, True),
    # ('bb', 'cc'): 51,997 matches; best class 5,897 docs, worst 7,000
    "bbcc-desc-k1": (5_897, False), "bbcc-desc-k10": (5_897, False),
    "bbcc-asc-k1": (7_000, False), "bbcc-asc-k10": (7_000, False),
    "bbcc-doc-k1": (51_997, True), "bbcc-doc-k10": (51_997, True),
}


def test_model_classes_unpruned():
    c = ref.classes_corpus()
    got = {cid: pick_model(narrow_keys(c, q, sort), k)
           for cid, (_, q, _, sort, k) in zip(NARROW_IDS, NARROW)}
    print(got)
    assert got == UNPRUNED_PATHS
    # both paths are there, with and without the tail copy
    assert any(fb for _, fb in got.values())
    assert any(not fb and n > S for n, fb in got.values())
    assert any(not fb and n <= S for n, fb in got.values())


def test_model_other_cases():
    tied = ref.tied_corpus()
    # one score for all 70,000: one bin, above T at any K
    assert pick_model(narrow_keys(tied, ref.AA, ref.SCORE_DESC), 65) == \
        (ref.N_BIG, True)
    # wide sort by u desc: the 100 docs at u64 max fill the top bin alone
    assert pick_model(wide_u_keys(tied, ref.AA, ref.DESC), 10) == (100, False)
    # sizes around S and T: n <= T keeps every record, T + 1 tied ones overflow
    for n in (S - 1, S, S + 1, T_MIN):
        keys = np.full(n, 0xC0 << 56, dtype=np.uint64) | np.arange(n, dtype=np.uint64)
        assert pick_model(keys, 10) == (n, False)
    c = ref.edge_corpus(T_MIN + 1)
    assert pick_model(narrow_keys(c, ALL, ref.SCORE_DESC), 10) == (T_MIN + 1, True)


# -------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def build_all():
    import __graft_entry__
    __graft_entry__.build()


class Pair:
    """A one-sync and a two-sync device context over the same splits."""

    def __init__(self, base):
        self.on = GpuSearcher(device=0, config=dict(base))
        self.off = GpuSearcher(device=0, config=dict(base, topk_onesync=False))
        self.loaded = set()

    def run(self, c, q, sort, max_hits, after=None):
        """{"on"/"off": (hits, one-sync calls, fallbacks, last survivors,
        last tail flag, last emitted)}; the two counts are this call's."""
        if c.split_id not in self.loaded:
            for s in (self.on, self.off):
                s.add_split(c.split_id, c.data)
            self.loaded.add(c.split_id)
        req = make_leaf_request(
            q.ast(), ref.SCHEMA, [(c.split_id, c.num_docs)], max_hits=max_hits,
            sort_fields=ref.sort_fields(sort) or None)
        if after is not None:
            req["search_request"]["search_after"] = after
        out = {}
        for tag, s in (("on", self.on), ("off", self.off)):
            before = s.topk_onesync_stats()
            try:
                resp = s.leaf_search(req)
            except RuntimeError as e:
                # a device error is not a mismatch: start nothing more
                pytest.exit(f"leaf_search failed, stopping the run: {e}", 3)
            now = s.topk_onesync_stats()
            out[tag] = (ref.hits_of(resp), now[0] - before[0],
                        now[1] - before[1], now[2], now[3], s.topk_stats()[2])
        return out


@pytest.fixture(scope="module")
def pruned(build_all):
    return Pair({})


@pytest.fixture(scope="module")
def unpruned(build_all):
    return Pair({"topk_prune": False})


FAST, FALLBACK, UNTOUCHED = (1, 0), (0, 1), (0, 0)


def check_both(pair, c, q, sort, k, path, what, exp=None, after=None):
    """Both contexts equal the reference; the default one took `path`, the
    two-sync one never counts. Returns the default context's record."""
    if exp is None:
        exp = ref.expected(c, q, sort, k)
    out = pair.run(c, q, sort, k, after)
    for tag in ("on", "off"):
        ref.assert_hits_exact(out[tag][0], exp, sort, (what, tag))
    print(what, "one-sync record", out["on"][1:])
    assert out["on"][1:3] == path, (what, out["on"][1:])
    assert out["off"][1:3] == UNTOUCHED, (what, out["off"][1:])
    return out["on"]


def check_survivors(rec, survivors):
    assert rec[3] == survivors
    assert rec[4] == int(survivors > S)


@pytest.mark.gpu
@pytest.mark.parametrize("qn,q,sn,sort,k", NARROW, ids=NARROW_IDS)
def test_narrow_pruned(pruned, qn, q, sn, sort, k):
    c = ref.classes_corpus()
    rec = check_both(pruned, c, q, sort, k, FAST, (qn, sn, k))
    emitted = rec[5]
    assert k <= emitted <= T_MIN  # module docstring: <= 2,880 in fact
    check_survivors(rec, emitted)


@pytest.mark.gpu
@pytest.mark.parametrize("qn,q,sn,sort,k", NARROW, ids=NARROW_IDS)
def test_narrow_unpruned(unpruned, qn, q, sn, sort, k):
    c = ref.classes_corpus()
    survivors, fallback = UNPRUNED_PATHS[f"{qn}-{sn}-k{k}"]
    rec = check_both(unpruned, c, q, sort, k, FALLBACK if fallback else FAST,
                     (qn, sn, k))
    assert rec[5] == ref.expected(c, q, sort, k)[0]  # every match a candidate
    if not fallback:
        check_survivors(rec, survivors)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [ref.DESC, ref.ASC], ids=["desc", "asc"])
def test_wide(pruned, order):
    """16-byte records: sort by the u64 column of the tied corpus. Descending,
    the 100 docs at u64 max have the top bin to themselves; ascending, the
    complements of 0, 1 and 2^32 (22,100 docs) share it and overflow T."""
    c = ref.tied_corpus()
    survivors, fallback = pick_model(wide_u_keys(c, ref.AA, order), 10)
    assert (survivors, fallback) == ((100, False) if order == ref.DESC
                                     else (22_100, True))
    rec = check_both(pruned, c, ref.AA, [("u", order)], 10,
                     FALLBACK if fallback else FAST, ("wide-u", order))
    if not fallback:
        check_survivors(rec, survivors)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [S - 1, S, S + 1, T_MIN, T_MIN + 1])
def test_sizes(unpruned, n):
    """n docs with one score, all candidates: n <= T keeps every record (the
    tail copy starts at S + 1), T + 1 tied records overflow one bin."""
    c = ref.edge_corpus(n)
    if n > T_MIN:
        check_both(unpruned, c, ALL, ref.SCORE_DESC, 10, FALLBACK, ("size", n))
        return
    rec = check_both(unpruned, c, ALL, ref.SCORE_DESC, 10, FAST, ("size", n))
    assert rec[3] == n
    assert rec[4] == int(n > S)


@pytest.mark.gpu
def test_tied_k65_falls_back(pruned):
    """K = 65 is outside the pruning gate: 70,000 candidates in one bin."""
    c = ref.tied_corpus()
    for sort in (ref.SCORE_DESC, ref.SCORE_ASC):
        rec = check_both(pruned, c, ref.AA, sort, 65, FALLBACK, ("tied", sort))
        assert rec[5] == c.num_docs


@pytest.mark.gpu
def test_search_after_untouched(pruned):
    c = ref.tied_corpus()
    sort = [("u", ref.DESC)]
    n, full = ref.ranked(c, ref.AA, sort)
    r = 1_500
    cur = ref.cursor_of(c, full[r], "u")
    check_both(pruned, c, ref.AA, sort, ref.AFTER_PAGE, UNTOUCHED, "after",
               exp=(n, full[r + 1:r + 1 + ref.AFTER_PAGE]), after=cur)


@pytest.mark.gpu
def test_empty_and_single(pruned, unpruned):
    c = ref.edge_corpus(8193)
    nothing = ref.Query(should=["all"], rng=("u", 100, 200))  # u = doc % 5
    one = ref.Query(must=["edge"], rng=("i", 8092, 8092))     # i = doc - 100
    assert ref.expected(c, nothing, ref.SCORE_DESC, 10) == (0, [])
    assert [h[0] for h in ref.expected(c, one, ref.SCORE_DESC, 10)[1]] == [8192]
    for pair in (pruned, unpruned):
        rec = check_both(pair, c, nothing, ref.SCORE_DESC, 10, FAST, "empty")
        check_survivors(rec, 0)
        rec = check_both(pair, c, one, ref.SCORE_DESC, 10, FAST, "single")
        check_survivors(rec, 1)
