"""Numpy model of the tile kernel's top-K pruning rule (kernels.hip, collection
phase of k_leaf_tile_t). No GPU, no native code.

The rule: a narrow candidate record is a u64 key, larger is better. A tile is
4 waves x 64 words; a word holds up to 32 docs. Per tile: each word's maximum
key (0 when empty), each wave's K-th largest word maximum, b = the largest of
the four wave values. One global u64 G holds the running maximum of every
tile's b (atomicMax). A tile emits the keys >= thr = max(G as it read it, b).

The kernel's comment argues that the emitted set always contains the exact
top-K, whatever order the tiles run in and however stale the G a tile reads.
This file is that argument made executable: tiles run in random orders, and in
the stale variant a tile sees ANY earlier value of G (0 included), which is
weaker than what atomicMax returns. Cases: random keys, heavy ties in the
upper key half (equal scores, the doc id decides), fewer than K matches
overall, and fewer than K non-empty words in every wave (the bound must stay
0 and nothing may be dropped).

The wave's K-th largest comes from a 64-lane bitonic network of shuffles;
test_bitonic_network runs the same compare-exchange schedule on numpy lanes.
"""
import numpy as np
import pytest

WORDS_PER_WAVE, WAVES, WORD_DOCS = 64, 4, 32
TILE_DOCS = WORDS_PER_WAVE * WAVES * WORD_DOCS  # 8192
KS = (1, 10, 64)


def bitonic_desc(v):
    """wave_sort_desc_u64 of kernels.hip: lane i ends with the i-th largest."""
    v = np.array(v, dtype=np.uint64)
    lane = np.arange(64)
    k = 2
    while k <= 64:
        j = k >> 1
        while j > 0:
            o = v[lane ^ j]
            keep_max = ((lane & j) == 0) == ((lane & k) == 0)
            v = np.where(keep_max, np.maximum(v, o), np.minimum(v, o))
            j >>= 1
        k <<= 1
    return v


def test_bitonic_network():
    rng = np.random.default_rng(1)
    for trial in range(200):
        if trial % 3 == 0:
            v = rng.integers(0, 4, 64).astype(np.uint64)  # heavy ties, zeros
        else:
            v = rng.integers(0, 2**63, 64).astype(np.uint64) * np.uint64(2) \
                + rng.integers(0, 2, 64).astype(np.uint64)
        assert (bitonic_desc(v) == np.sort(v)[::-1]).all()


def tile_bound(keys, match, k):
    """b of one tile. keys/match: [TILE_DOCS]."""
    km = np.where(match, keys, np.uint64(0)).reshape(
        WAVES, WORDS_PER_WAVE, WORD_DOCS)
    wmax = km.max(axis=2)
    return max(int(bitonic_desc(wmax[w])[k - 1]) for w in range(WAVES))


def run_tiles(keys, match, k, order, stale_rng=None):
    """Emitted doc mask after the tiles ran in `order`. With stale_rng, each
    tile reads any earlier value of G instead of the current one."""
    n_tiles = len(keys) // TILE_DOCS
    emitted = np.zeros(len(keys), dtype=bool)
    history = [0]  # every value G has held
    for t in order:
        sl = slice(t * TILE_DOCS, (t + 1) * TILE_DOCS)
        b = tile_bound(keys[sl], match[sl], k)
        seen = history[-1] if stale_rng is None else \
            history[int(stale_rng.integers(0, len(history)))]
        history.append(max(history[-1], b))
        thr = max(seen, b)
        emitted[sl] = match[sl] & (keys[sl] >= np.uint64(thr))
    assert len(history) == n_tiles + 1
    return emitted


def make_keys(rng, n_tiles, kind):
    """Distinct u64 keys (the low half is the doc id, as in the kernel) and a
    match mask."""
    n = n_tiles * TILE_DOCS
    doc = np.arange(n, dtype=np.uint64)
    if kind == "random":
        hi = rng.integers(1, 2**31, n).astype(np.uint64)
        match = rng.random(n) < 0.25
    elif kind == "ties":  # three score classes, ~25% density
        hi = rng.choice(np.array([7, 8, 9], dtype=np.uint64), n)
        match = rng.random(n) < 0.25
    elif kind == "all-tied-dense":  # one score everywhere, every doc matches
        hi = np.full(n, 5, dtype=np.uint64)
        match = np.ones(n, dtype=bool)
    elif kind == "few-matches":  # fewer than K = 10 / 64 matches overall
        hi = rng.integers(1, 2**31, n).astype(np.uint64)
        match = np.zeros(n, dtype=bool)
        match[rng.choice(n, 7, replace=False)] = True
    elif kind == "sparse-words":  # < K non-empty words per wave for K >= 10
        hi = rng.integers(1, 2**31, n).astype(np.uint64)
        match = np.zeros(n, dtype=bool)
        words = match.reshape(-1, WORDS_PER_WAVE, WORD_DOCS)
        for wave in words:  # 9 full words per wave: many docs, few words
            wave[rng.choice(WORDS_PER_WAVE, 9, replace=False)] = True
    else:
        raise AssertionError(kind)
    return (hi << np.uint64(32)) | doc, match


KINDS = ("random", "ties", "all-tied-dense", "few-matches", "sparse-words")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", KS)
def test_emitted_contains_topk(kind, k):
    rng = np.random.default_rng(100 * KINDS.index(kind) + k)
    n_tiles = 6
    keys, match = make_keys(rng, n_tiles, kind)
    matched = np.nonzero(match)[0]
    top = matched[np.argsort(keys[matched])[::-1][:k]]
    orders = [np.arange(n_tiles), np.arange(n_tiles)[::-1]] + \
        [rng.permutation(n_tiles) for _ in range(4)]
    for order in orders:
        for stale in (None, np.random.default_rng(3)):
            em = run_tiles(keys, match, k, order, stale)
            assert em[top].all(), (kind, k, list(order), stale is not None)
            assert not (em & ~match).any()
            assert em.sum() >= min(k, len(matched))
    if kind == "sparse-words" and k >= 10:
        # every wave has 9 non-empty words: all bounds 0, nothing pruned
        assert (run_tiles(keys, match, k, orders[0]) == match).all()
    if kind == "few-matches" and k >= 10:
        assert (run_tiles(keys, match, k, orders[0]) == match).all()


def test_prunes_something():
    """The rule is not vacuous: on dense random keys the emitted set is a
    small fraction of the matches."""
    rng = np.random.default_rng(9)
    keys, match = make_keys(rng, 6, "random")
    em = run_tiles(keys, match, 10, np.arange(6))
    assert em.sum() < match.sum() // 10
