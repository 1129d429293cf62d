"""Corpora and ground truth for the posting-block decoders.

Plain helper module (not a conftest): numpy, quickwit_amd.splitgen,
quickwit_amd.splitread, topk_reference (quantize_lengths, K1, B, REL) and
phrase_window_reference. Nothing from the oracle or the product.
test_posting_decode_cpu.py proves it (writer, reader, oracle) without a GPU;
test_posting_decode_gpu.py then holds the four device decoders to it.

The ground truth of a term is the (doc_ids, tfs) arrays chosen here. A block
of the format holds 128 postings, bitpacked at id_bits per gap and tf_bits
per tf - 1; realised() reads the widths the writer actually chose back from
the split, so that the tests can prove each case is what it claims to be.

Corpus A, "widths": 4,194,304 docs, explicit posting lists, no tokens.
  field pf (record freq, fieldnorms), terms:
    g01..g22   one full block with id_bits == w, then a partial block. As
               many gaps as the doc-id space allows have bit w-1 set, at
               least one per 32-posting segment (w <= 19; two for w = 20,
               21 and one for w = 22, which is all that fits), at lanes
               that differ between terms. tf in 1..3.
    fWWn fWWw  one full block with tf_bits == WW (1..20): tf - 1 uniform in
               [0, 2^WW), top bit set in over a quarter. The n variant has
               id_bits <= 16, the w variant id_bits == 17, so the tf
               section starts at two different offsets.
    cNNNn      exactly NNN postings, gaps of at most 3 bits
    cNNNw      the same counts with id_bits == 17 in every block that has a
               gap (a block of one posting has none: id_bits 1)
    e0 e1      tile edges: docs {0, 8191, 8192, 16383, N-1}; a full block
               that starts in tile 0 and ends in tile 1
    p0         26 blocks overlap tile 300, 25 of them inside it;
               consecutive blocks differ in id_bits and in tf_bits (1..13)
    p1         in tile 20: a block arriving by a gap >= 65,536, eight dense
               blocks (id_bits <= 2), a block leaving by a gap >= 65,536
    u0         every third posting of each term above plus docs of its own:
               the partner of the must / must_not cases
  field pb (record basic, no fieldnorms): the c* doc lists; tf_bits == 0.
  Doc length = sum of tf over the doc's terms.

ORDER. A single-term score list is in a determined order only if no two
different float64 scores are closer than the device's f32 arithmetic can
tell apart. W * tf / (tf + K) in f32 is four roundings, at most 2.4e-7
relative, so two scores 5e-7 apart cannot swap. The generator redraws the
free tfs (f*, p0, p1) until any two different scores of one term are at
least MIN_SEP = 2e-6 apart relative, or bit-equal (same tf, same quantized
length: the same f32 operations, tie broken by doc id). The CPU test
asserts the separation, so the exact-order assertion of the GPU test stands
on the reference alone.

Corpus B, "phrase": 200,000 docs through SplitWriter (record position),
all but a few hundred empty. Pair k has tokens (xKK, yKK); one of the two
(the "exact" token, x for pairs 0-8, y for 9-17) has a posting list built
to a given count, id_bits and tf_bits; the other token misses every eighth
of those docs and has three docs of its own. Doc kinds, by position in the
exact token's list: "x y" (four in eight), "x fil y", "y x", exact token
alone, "x fil*5 y". Ground truth is phrase_window_reference's brute force.
"""
import functools
import math

import numpy as np

import phrase_window_reference as pref
from quickwit_amd import splitgen, splitread
from topk_reference import B, K1, REL, quantize_lengths  # noqa: F401

BLOCK = 128
TILE_DOCS = 8192
MIN_SEP = 2e-6

# ---------------------------------------------------------------- corpus A
N_A = 1 << 22
PF, PB = "pf", "pb"
SCHEMA_A = {"timestamp_field": None, "fields": [
    {"name": PF, "type": "text", "tokenizer": "raw", "record": "freq",
     "fieldnorms": True},
    {"name": PB, "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False}]}
SPLIT_A = "posting-widths"

GAP_WIDTHS = list(range(1, 23))
TF_WIDTHS = list(range(1, 21))
COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256,
          257]
P0_TILE, P1_TILE = 300, 20
# id_bits of p0's blocks: the first arrives from below the tile, the last
# has the widest gap; those between lie inside (wide gaps sum to about 3,000)
P0_ID_BITS = [13, 1, 5, 2, 9, 3, 7, 1, 10, 4, 6, 2, 8, 1, 11, 3, 5, 2, 7, 4,
              6, 1, 9, 2, 3, 12]
P0_TF_BITS = [(7 * i + 3) % 13 + 1 for i in range(len(P0_ID_BITS))]
P1_ID_BITS = [17, 1, 2, 1, 2, 1, 2, 1, 2, 17]
P1_TF_BITS = [2, 5, 1, 3, 6, 2, 4, 1, 3, 5]
# segments of a full block that get a gap with the top bit set, where 128
# (or even four) such gaps do not fit into 2^22 docs
WIDE_SEGS = {17: 4, 18: 4, 19: 4, 20: 2, 21: 2, 22: 1}


def _top_lanes(w, count, n_top, rng):
    """Lanes (1..count-1) of the gaps that get bit w-1: one per 32-posting
    segment first, at a lane that depends on w, then random others."""
    lanes = []
    for s in ((w + i) % 4 for i in range(4)):
        lo, hi = max(32 * s, 1), min(32 * s + 32, count)
        if lo < hi and len(lanes) < n_top:
            lanes.append(lo + (5 * w + 11 * s) % (hi - lo))
    rest = [j for j in range(1, count) if j not in lanes]
    extra = min(max(n_top - len(lanes), 0), len(rest))
    if extra:
        lanes += rng.choice(rest, size=extra, replace=False).tolist()
    return sorted(lanes)


def _block_gaps(rng, w, count=BLOCK, n_top=None, other_hi=None, top_span=None):
    """gaps[0..count): gaps[0] = 0 (posting 0 is the block's first doc); the
    block's id_bits is exactly w (count >= 2)."""
    g = np.ones(count, dtype=np.int64)
    if w > 1 and count > 1:
        lo = 1 << (w - 1)
        span = lo if top_span is None else min(top_span, lo)
        if n_top is None:
            n_top = count - 1
        other_hi = min(other_hi or (1 << w), 1 << w)
        g = rng.integers(1, max(other_hi, 2), size=count).astype(np.int64)
        lanes = _top_lanes(w, count, max(n_top, 1), rng)
        g[lanes] = lo + rng.integers(0, span, size=len(lanes))
    g[0] = 0
    return g


def _docs_from(first, gaps):
    return first + np.cumsum(gaps)


class CorpusA:
    def __init__(self):
        self.num_docs = N_A
        self.split_id = SPLIT_A
        self.terms = {PF: {}, PB: {}}   # term -> (docs i64, tfs i64)
        self._free = {}                 # pf term -> (lo, hi) tf - 1 ranges
        self._build()
        self._separate()
        self._data = None
        self._cache = {}

    # ---- construction
    def _add(self, term, docs, tfs, field=PF, free=None):
        docs = np.asarray(docs, dtype=np.int64)
        tfs = np.asarray(tfs, dtype=np.int64)
        assert len(docs) == len(tfs) and (np.diff(docs) > 0).all(), term
        assert 0 <= docs[0] and docs[-1] < self.num_docs, (term, docs[-1])
        assert term not in self.terms[field]
        self.terms[field][term] = (docs, tfs)
        if free is not None:
            self._free[term] = free

    def _build(self):
        rng = np.random.default_rng(20240607)
        g_docs = {}
        for w in GAP_WIDTHS:
            if w >= 17:
                gaps = _block_gaps(rng, w, n_top=WIDE_SEGS[w], other_hi=1 << 10,
                                   top_span=1 << (w - 3))
                first = int(rng.integers(0, 1 << 16))
            else:
                # bit w-1 in as many gaps as fit into about 2^21 docs
                n_top = min(BLOCK - 1, (1 << 21) // (3 << (w - 1) >> 1))
                gaps = _block_gaps(rng, w, n_top=n_top, other_hi=1 << 12)
                first = int(rng.integers(0, 1 << 20))
            part = _block_gaps(rng, min(w, 6), count=40 + w)
            part[0] = 1 + int(rng.integers(0, 50))  # gap between the blocks
            docs = _docs_from(first, np.concatenate([gaps, part]))
            self._add("g%02d" % w, docs, rng.integers(1, 4, size=len(docs)))
            g_docs[w] = docs

        def anchor(t, k):
            """A doc of the t-th g term, so that the anchored term shares at
            least that doc with it; low enough to leave room for the term."""
            d = g_docs[GAP_WIDTHS[t % len(GAP_WIDTHS)]]
            for j in (k, 7, 1, 0):
                if d[j] < self.num_docs - 400_000:
                    return int(d[j])
            raise AssertionError("no room")

        self.f_terms = []
        t = 0
        for w in TF_WIDTHS:
            for variant in "nw":
                if variant == "n":
                    idw = 1 + (3 * w) % 16
                    gaps = _block_gaps(rng, idw, n_top=4, other_hi=1 << 4)
                else:
                    gaps = _block_gaps(rng, 17, n_top=1, other_hi=1 << 4,
                                       top_span=1 << 13)
                docs = _docs_from(anchor(t, 10 + 50 * (t // 22)), gaps)
                lo = np.zeros(BLOCK, dtype=np.int64)
                hi = np.full(BLOCK, (1 << w) - 1, dtype=np.int64)
                lo[1::4] = 1 << (w - 1)  # top bit forced in a quarter
                tf1 = rng.integers(lo, hi + 1)
                name = "f%02d%s" % (w, variant)
                self._add(name, docs, tf1 + 1, free=(lo, hi))
                self.f_terms.append(name)
                t += 1

        self.c_terms = []
        t = 0
        for variant in "nw":
            for n in COUNTS:
                gaps = []
                for b in range(0, n, BLOCK):
                    cnt = min(BLOCK, n - b)
                    if variant == "n":
                        g = rng.integers(1, 8, size=cnt).astype(np.int64)
                    else:
                        g = _block_gaps(rng, 17, count=cnt, n_top=1,
                                        other_hi=1 << 3, top_span=1 << 12)
                    g[0] = 0 if b == 0 else 1 + int(rng.integers(0, 5))
                    gaps.append(g)
                docs = _docs_from(anchor(t, 20 + 50 * (t // 22)),
                                  np.concatenate(gaps))
                name = "c%03d%s" % (n, variant)
                self._add(name, docs, rng.integers(1, 4, size=n))
                self._add(name, docs, np.ones(n, dtype=np.int64), field=PB)
                self.c_terms.append(name)
                t += 1

        self._add("e0", [0, TILE_DOCS - 1, TILE_DOCS, 2 * TILE_DOCS - 1,
                         self.num_docs - 1], [1, 3, 2, 1, 2])
        self._add("e1", TILE_DOCS - 64 + np.arange(BLOCK),
                  rng.integers(1, 4, size=BLOCK))

        # p0: blocks of alternating widths over one tile
        lo_doc = P0_TILE * TILE_DOCS
        docs, tf_lo, tf_hi = [], [], []
        cur = lo_doc - 4100
        for b, (iw, tw) in enumerate(zip(P0_ID_BITS, P0_TF_BITS)):
            g = np.ones(BLOCK, dtype=np.int64)
            if iw > 1:
                lane = 1 + (17 * b + 5) % (BLOCK - 1)
                if b == 0:
                    lane = 20   # 20 postings below the tile, the rest inside
                g[lane] = (1 << (iw - 1)) + int(
                    rng.integers(0, max(1 << (iw - 1) >> 3, 1)))
            g[0] = 1  # the gap between two blocks is not stored
            d = cur + np.cumsum(g)
            cur = int(d[-1])
            docs.append(d)
            l = np.zeros(BLOCK, dtype=np.int64)
            l[(3 * b) % BLOCK] = 1 << (tw - 1)
            tf_lo.append(l)
            tf_hi.append(np.full(BLOCK, (1 << tw) - 1, dtype=np.int64))
        docs, tf_lo, tf_hi = map(np.concatenate, (docs, tf_lo, tf_hi))
        self._add("p0", docs, rng.integers(tf_lo, tf_hi + 1) + 1,
                  free=(tf_lo, tf_hi))

        # p1: wide, eight dense, wide within one tile
        lo_doc = P1_TILE * TILE_DOCS
        docs, tf_lo, tf_hi = [], [], []
        cur = lo_doc - 70_000
        for b, (iw, tw) in enumerate(zip(P1_ID_BITS, P1_TF_BITS)):
            g = np.ones(BLOCK, dtype=np.int64)
            if iw == 17:
                g[64] = 70_100 if b == 0 else 66_000 + int(rng.integers(0, 999))
            elif iw == 2:
                g[1:] = rng.integers(1, 4, size=BLOCK - 1)
                g[1 + b] = 3
            g[0] = 1 + b % 3
            d = cur + np.cumsum(g)
            cur = int(d[-1])
            docs.append(d)
            l = np.zeros(BLOCK, dtype=np.int64)
            l[(5 * b + 2) % BLOCK] = 1 << (tw - 1)
            tf_lo.append(l)
            tf_hi.append(np.full(BLOCK, (1 << tw) - 1, dtype=np.int64))
        docs, tf_lo, tf_hi = map(np.concatenate, (docs, tf_lo, tf_hi))
        self._add("p1", docs, rng.integers(tf_lo, tf_hi + 1) + 1,
                  free=(tf_lo, tf_hi))

        shared = [d[::3] for d, _ in self.terms[PF].values()]
        own = 1000 + 997 * np.arange(500)
        u0 = np.unique(np.concatenate(shared + [own]))
        self._add("u0", u0, np.ones(len(u0), dtype=np.int64))
        shared = [d[::3] for d, _ in self.terms[PB].values()]
        u0 = np.unique(np.concatenate(shared + [own]))
        self._add("u0", u0, np.ones(len(u0), dtype=np.int64), field=PB)

    def _lengths(self, field):
        n = np.zeros(self.num_docs, dtype=np.int64)
        for docs, tfs in self.terms[field].values():
            np.add.at(n, docs, tfs)
        return n

    def _weight(self, term):
        df = len(self.terms[PF][term][0])
        return math.log(1.0 + (self.num_docs - df + 0.5) / (df + 0.5)) \
            * (1.0 + K1)

    def _near_ties(self, group, lengths, avgdl):
        """[(term, posting)] of one posting out of every two of the group's
        terms whose float64 scores differ, but by less than MIN_SEP
        relative; the redrawable one of the two where there is one."""
        s, who = [], []
        for t in group:
            docs, tfs = self.terms[PF][t]
            s.append(_bm25(tfs, quantize_lengths(lengths[docs]), avgdl,
                           self._weight(t)))
            who += [(t, i) for i in range(len(docs))]
        s = np.concatenate(s)
        order = np.argsort(s, kind="stable")
        d = np.diff(s[order])
        out = []
        for i in np.nonzero((d > 0) & (d < MIN_SEP * s[order][1:]))[0]:
            pair = [who[order[i]], who[order[i + 1]]]
            free = [(t, k) for t, k in pair if t in self._free
                    and self._free[t][1][k] > self._free[t][0][k]]
            out.append((free or pair)[0])
        return out

    def _separate(self):
        """Redraw free tfs until the scores of every term (and of p0 and p1
        together, for the two-term case) are MIN_SEP apart or equal (module
        docstring, ORDER). Deterministic."""
        rng = np.random.default_rng(77)
        groups = [[t] for t in self._free] + [["p0", "p1"]]
        for _ in range(400):
            lengths = self._lengths(PF)
            avgdl = float(lengths.sum()) / self.num_docs
            moved = 0
            for group in groups:
                for t, k in self._near_ties(group, lengths, avgdl):
                    if t in self._free:
                        lo, hi = self._free[t]
                        if hi[k] > lo[k]:
                            self.terms[PF][t][1][k] = \
                                int(rng.integers(lo[k], hi[k] + 1)) + 1
                            moved += 1
            if not moved:
                return
        raise AssertionError("tf redraw did not settle")

    # ---- the split image
    @property
    def data(self):
        if self._data is None:
            pre = {}
            for field in (PF, PB):
                vocab = sorted(self.terms[field])
                tid, did, tf = [], [], []
                for i, t in enumerate(vocab):
                    docs, tfs = self.terms[field][t]
                    tid.append(np.full(len(docs), i, dtype=np.int64))
                    did.append(docs.astype(np.uint32))
                    tf.append(tfs.astype(np.uint32))
                pre[field] = (vocab, np.concatenate(tid), np.concatenate(did),
                              np.concatenate(tf), self._lengths(field))
            self._data = splitgen._assemble(SCHEMA_A, self.split_id,
                                            self.num_docs, {}, {},
                                            precomputed_text=pre)
        return self._data

    # ---- ground truth
    def postings(self, field, term):
        return self.terms[field][term]

    def doc_set(self, field, term):
        return set(self.terms[field][term][0].tolist())

    def scores64(self, field, term):
        """float64 BM25 of each posting of a one-term query
        (topk_reference.scores64's formula)."""
        key = ("s", field, term)
        if key not in self._cache:
            docs, tfs = self.terms[field][term]
            if "len" + field not in self._cache:
                self._cache["len" + field] = self._lengths(field)
            lengths = self._cache["len" + field]
            avgdl = float(lengths.sum()) / self.num_docs
            # a field without fieldnorms scores every doc at length 1
            qlen = quantize_lengths(lengths[docs]) if field == PF \
                else np.ones(len(docs), dtype=np.int64)
            df = len(docs)
            idf = math.log(1.0 + (self.num_docs - df + 0.5) / (df + 0.5))
            self._cache[key] = _bm25(tfs, qlen, avgdl, idf * (1.0 + K1))
        return self._cache[key]

    def ranked(self, field, terms):
        """[(doc, score)] of a `should` of one or two terms, by score
        descending, ties by doc id descending (topk_reference.ranked)."""
        total = {}
        for t in terms:
            for d, s in zip(self.terms[field][t][0].tolist(),
                            self.scores64(field, t).tolist()):
                total[d] = total.get(d, 0.0) + s
        return sorted(total.items(), key=lambda ds: (-ds[1], -ds[0]))

    def min_separation(self, field, term):
        """Smallest relative distance of two different scores of the term."""
        s = np.unique(self.scores64(field, term))
        return float((np.diff(s) / s[1:]).min()) if len(s) > 1 else math.inf


def _bm25(tfs, qlen, avgdl, weight):
    tf = np.asarray(tfs, dtype=np.float64)
    kd = K1 * (1.0 - B + B * np.asarray(qlen, dtype=np.float64)
               / (avgdl if avgdl > 0 else 1.0))
    return weight * tf / (tf + kd)


@functools.lru_cache(maxsize=None)
def corpus_a():
    return CorpusA()


def realised(data, field):
    """{term: [(id_bits, tf_bits, count) of each of its blocks]}, read back
    from the split image."""
    s = splitread.Split(data)
    skip = s._sec(field, "skip", splitgen.SKIP_DTYPE)
    n_blocks = s._sec(field, "n_blocks", "<u4")
    skip_off = s._sec(field, "skip_off", "<u8")
    out = {}
    for i, t in enumerate(s.terms(field)):
        first = int(skip_off[i]) // 16
        out[t] = [(int(e["id_bits"]), int(e["tf_bits"]), int(e["count"]))
                  for e in skip[first:first + int(n_blocks[i])]]
    return out


def block_ranges(data, field, term):
    """[(first_doc, last_doc)] of the term's blocks."""
    s = splitread.Split(data)
    tid = s.term_id(field, term)
    skip = s._sec(field, "skip", splitgen.SKIP_DTYPE)
    first = int(s._sec(field, "skip_off", "<u8")[tid]) // 16
    n = int(s._sec(field, "n_blocks", "<u4")[tid])
    return [(int(e["first_doc"]), int(e["last_doc"]))
            for e in skip[first:first + n]]


def term_query(term, field=PF):
    return {"type": "term", "field": field, "value": term}


def regex_query(pattern, field=PF):
    return {"type": "regex", "field": field, "regex": pattern}


# requests shared by the CPU and the GPU file ------------------------------
def scored_terms():
    """[(field, term)] of the one-term scored cases."""
    a = corpus_a()
    return [(PF, t) for t in sorted(a.terms[PF]) if t != "u0"] + \
           [(PB, t) for t in sorted(a.terms[PB]) if t != "u0"]


def count_role_cases():
    """[(g, f, c)]: a should of three with minimum_should_match 2. f and c
    were anchored on a doc of g (CorpusA._build), so no case is empty."""
    a = corpus_a()
    g = ["g%02d" % w for w in GAP_WIDTHS]
    return [(g[t % len(g)], a.f_terms[t], a.c_terms[t % len(a.c_terms)])
            for t in range(len(a.f_terms))]


def count_role_expected(case):
    a = corpus_a()
    sets = [a.doc_set(PF, t) for t in case]
    return sorted(d for d in set().union(*sets)
                  if sum(d in s for s in sets) >= 2)


def bitset_terms():
    """[(field, term)] decoded once as must and once as must_not, against
    the partner that shares every third posting with it."""
    a = corpus_a()
    return [(PF, t) for t in sorted(a.terms[PF])
            if t[0] in "gcpe"] + [(PB, t) for t in sorted(a.terms[PB])
                                  if t != PARTNER]


PARTNER = "u0"  # in both fields: every third posting of each other term


def bool_query(field, must, must_not):
    return {"type": "bool", "must": [term_query(must, field)],
            "must_not": [term_query(must_not, field)]}


def union_patterns():
    """[(pattern, [terms it matches])] on pf."""
    a = corpus_a()
    names = sorted(a.terms[PF])
    one = [(t, [t]) for t in names if t[0] in "gc"]
    return one + [
        ("g[0-9]+", [t for t in names if t[0] == "g"]),
        ("c[0-9]+[nw]", [t for t in names if t[0] == "c"]),
        ("f[0-9]+[nw]", [t for t in names if t[0] == "f"]),
        (".*", names)]


def union_expected(terms):
    a = corpus_a()
    return sorted(set().union(*[a.doc_set(PF, t) for t in terms]))


# ---------------------------------------------------------------- corpus B
N_B = 200_000
SPLIT_B = "posting-phrase"
SCHEMA_B = {"timestamp_field": None, "fields": [
    {"name": "body", "type": "text", "tokenizer": "default",
     "record": "position", "fieldnorms": True}]}
FIL = "fil"
# (count, id_bits, tf_bits) of the exact token's list, pair by pair. A list
# of one posting has no gap: id_bits 1. tf_bits 16 and 17 (one doc holding
# the token 40,001 and 65,537 times) occur once per role and no wider: the
# kernels loop over tf.
PAIR_SPECS = [(1, 1, 1), (32, 2, 3), (33, 5, 8), (64, 8, 9), (65, 9, 1),
              (96, 12, 3), (97, 16, 16), (128, 17, 17), (129, 18, 8)]
SLOPS = (0, 1, 3)


def _pair_tokens(k):
    return "x%02d" % k, "y%02d" % k


class CorpusB:
    def __init__(self):
        rng = np.random.default_rng(4242)
        self.num_docs = N_B
        self.split_id = SPLIT_B
        toks = {}  # doc -> token list

        def put(d, seq):
            assert 0 <= d < N_B, d
            toks.setdefault(int(d), []).extend(seq)

        self.pairs = []
        for k in range(2 * len(PAIR_SPECS)):
            count, idw, tfw = PAIR_SPECS[k % len(PAIR_SPECS)]
            x, y = _pair_tokens(k)
            exact, other = (x, y) if k < len(PAIR_SPECS) else (y, x)
            gaps = []
            for b in range(0, count, BLOCK):
                cnt = min(BLOCK, count - b)
                g = _block_gaps(rng, idw if cnt > 1 else 1, count=cnt,
                                n_top=1 if idw >= 12 else 3,
                                other_hi=1 << min(idw, 3), top_span=1 << 9)
                g[0] = 0 if b == 0 else 2
                gaps.append(g)
            docs = _docs_from(int(rng.integers(0, 20_000)),
                              np.concatenate(gaps))
            big = count // 3  # the posting that realises tf_bits
            for i, d in enumerate(docs.tolist()):
                reps = 1
                if i == big and tfw > 1:
                    reps = {16: 40_001, 17: 65_537}.get(tfw, (1 << (tfw - 1)) + 2)
                elif i == big:
                    reps = 2
                elif tfw >= 3 and i % 8 < 4:
                    reps = int(rng.integers(1, 6))
                xs = [x] * (reps if exact == x else 1)
                ys = [y] * (reps if exact == y else 1)
                kind = 0 if i == big else i % 8
                if kind < 4:
                    put(d, xs + ys)
                elif kind == 4:
                    put(d, xs + [FIL] + ys)
                elif kind == 5:
                    put(d, ys + xs)
                elif kind == 6:
                    put(d, [exact, FIL])
                else:
                    put(d, xs + [FIL] * 5 + ys)
            taken = set(docs.tolist())
            alone = [d + 1 for d in docs.tolist() if d + 1 not in taken][:3]
            for d in alone:
                put(d, [FIL, other])
            self.pairs.append((x, y))
        self.toks = toks
        self.docs = sorted(toks)
        self.vocab = sorted({t for seq in toks.values() for t in seq})
        self._sets = {d: set(seq) for d, seq in toks.items()}
        self._data = None
        self._cache = {}

    @property
    def data(self):
        if self._data is None:
            w = splitgen.SplitWriter(SCHEMA_B, self.split_id, store_docs=False)
            w.add_documents([{"body": " ".join(self.toks[d])} if d in self.toks
                             else {} for d in range(self.num_docs)])
            self._data = w.finalize()
        return self._data

    def postings(self, tok):
        docs = [d for d in self.docs if tok in self._sets[d]]
        return (np.array(docs, dtype=np.int64),
                np.array([self.toks[d].count(tok) for d in docs],
                         dtype=np.int64))

    # brute force, over the docs that hold the first token at all (a doc
    # without it matches nothing)
    def slop_hits(self, phrase, slop):
        key = (tuple(phrase), slop)
        if key not in self._cache:
            self._cache[key] = [
                d for d in self.docs if phrase[0] in self._sets[d]
                and pref.slop_match(self.toks[d], list(phrase), slop)]
        return self._cache[key]

    def prefix_hits(self, phrase, max_expansions=50):
        exps = pref.expansions([self.vocab], phrase[-1], max_expansions)
        hits = set()
        for e in exps:
            hits.update(self.slop_hits(list(phrase[:-1]) + [e], 0))
        return sorted(hits)


@functools.lru_cache(maxsize=None)
def corpus_b():
    return CorpusB()


def slop_query(toks, slop):
    mode = {"type": "phrase"}
    if slop:
        mode["slop"] = slop
    return {"type": "full_text", "field": "body", "text": " ".join(toks),
            "params": {"mode": mode}}


def prefix_query(toks, max_expansions=50):
    return {"type": "phrase_prefix", "field": "body", "phrase": " ".join(toks),
            "max_expansions": max_expansions,
            "params": {"mode": {"type": "phrase"}}, "lenient": False}


def hit_ids(resp):
    """A hit on doc 0 carries no doc_id key."""
    return [h.get("doc_id", 0) for h in resp.get("partial_hits", [])]


# ------------------------------------------- the requests of both test files
def cases_a():
    """[(id, query ast, "scored" | "set", expected)] on corpus A. scored:
    sort by _score descending, expected = [(doc, score64)] in order, every
    posting returned. set: unsorted, expected = sorted doc ids."""
    a = corpus_a()
    out = []
    for field, t in scored_terms():
        out.append(("scored-%s-%s" % (field, t), term_query(t, field),
                    "scored", a.ranked(field, [t])))
    out.append(("scored-pf-p0+p1",
                {"type": "bool", "should": [term_query("p0"),
                                            term_query("p1")]},
                "scored", a.ranked(PF, ["p0", "p1"])))
    for case in count_role_cases():
        out.append(("count-" + "-".join(case),
                    {"type": "bool", "should": [term_query(t) for t in case],
                     "minimum_should_match": 2},
                    "set", count_role_expected(case)))
    for field, t in bitset_terms():
        mine, other = a.doc_set(field, t), a.doc_set(field, PARTNER)
        # a term of one posting shares it: its must case expects nothing
        assert mine & other and other - mine and \
            (mine - other or len(mine) == 1), (field, t)
        out.append(("must-%s-%s" % (field, t), bool_query(field, t, PARTNER),
                    "set", sorted(mine - other)))
        out.append(("must_not-%s-%s" % (field, t),
                    bool_query(field, PARTNER, t), "set",
                    sorted(other - mine)))
    return out


def cases_union():
    return [("union-" + p, regex_query(p), "set", union_expected(terms))
            for p, terms in union_patterns()]


def cases_b():
    """[(id, query ast, "set", expected)] on corpus B: every pair at each
    slop and as a two-token phrase prefix."""
    b = corpus_b()
    out = []
    for x, y in b.pairs:
        for s in SLOPS:
            out.append(("phrase-%s-slop%d" % (x, s), slop_query([x, y], s),
                        "set", b.slop_hits([x, y], s)))
        out.append(("prefix-" + x, prefix_query([x, y[:-1]]), "set",
                    b.prefix_hits([x, y[:-1]])))
    return out


def check_response(resp, kind, expected, what):
    """num_hits, ids (in order when scored) exact; scores within REL.
    Returns the largest relative score deviation."""
    assert not resp.get("failed_splits"), (what, resp.get("failed_splits"))
    assert resp.get("num_hits", 0) == len(expected), \
        (what, "num_hits", resp.get("num_hits", 0), len(expected))
    ids = hit_ids(resp)
    if kind == "set":
        assert sorted(ids) == expected, (what, "doc set")
        return 0.0
    want = [d for d, _ in expected]
    if ids != want:
        assert len(ids) == len(want), (what, "hit count", len(ids), len(want))
        r = next(i for i, (g, e) in enumerate(zip(ids, want)) if g != e)
        raise AssertionError("%s: ids differ first at rank %d: got %d, want %d"
                             % (what, r, ids[r], want[r]))
    worst = 0.0
    for h, (d, s) in zip(resp["partial_hits"], expected):
        dev = abs(h["sort_value"]["f64"] - s) / s
        worst = max(worst, dev)
        assert dev <= REL, (what, "score", d, h["sort_value"]["f64"], s)
    return worst
