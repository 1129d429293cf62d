"""Proves tests/posting_reference.py before a GPU is involved: the corpora
realise exactly the block widths and counts they claim (read back from the
split image), the numpy reader returns the generator's arrays for every term
(writer and reader, no C++), scores of one term are far enough apart for
their order to be determined, and the oracle answers every request of
test_posting_decode_gpu.py with the reference's doc ids, num_hits and order,
scores within topk_reference.REL. The oracle has no regex, sloppy-phrase or
phrase-prefix evaluation; for those requests the reference is the union of
generator arrays and phrase_window_reference's brute force (proved by
test_phrase_window_cpu.py), and the oracle is asked the slop-0 phrases only.

The width and count sets are asserted as EXACT sets: if the writer or the
generator changes so that a case no longer is what it claims, this fails.
"""
import numpy as np
import pytest

import posting_reference as ref
from quickwit_amd import splitread
from quickwit_amd.api import OracleSearcher, make_leaf_request


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


@pytest.fixture(scope="module")
def real_a():
    data = ref.corpus_a().data
    return {f: ref.realised(data, f) for f in (ref.PF, ref.PB)}


@pytest.fixture(scope="module")
def real_b():
    return ref.realised(ref.corpus_b().data, "body")


# ------------------------------------------------------ what the corpora are
def test_gap_and_tf_widths_are_exactly_the_claimed_sets(real_a):
    pf, pb = real_a[ref.PF], real_a[ref.PB]
    for w in ref.GAP_WIDTHS:
        blocks = pf["g%02d" % w]
        assert blocks[0] == (w, 2, 128) and len(blocks) == 2, (w, blocks)
        assert 0 < blocks[1][2] < 128
    for w in ref.TF_WIDTHS:
        (lo,), (hi,) = pf["f%02dn" % w], pf["f%02dw" % w]
        assert lo[1:] == (w, 128) and hi == (17, w, 128), (w, lo, hi)
        assert lo[0] == 1 + (3 * w) % 16 <= 16
    assert {b[0] for t in pf for b in pf[t] if t[0] == "g"} == \
        set(range(1, 23))
    assert {b[0] for bl in pf.values() for b in bl} == set(range(1, 23))
    assert {b[1] for bl in pf.values() for b in bl} == set(range(1, 21))
    assert {b[1] for bl in pb.values() for b in bl} == {0}
    # the tf section's start offset 2 * ((128 * id_bits + 63) / 64) under
    # both arms of the gap decoder, for every tf width
    for w in ref.TF_WIDTHS:
        ids = {b[0] for v in "nw" for b in pf["f%02d%s" % (w, v)]}
        assert min(ids) <= 16 < max(ids)


def test_top_bit_gaps_sit_in_every_segment_at_differing_lanes():
    a = ref.corpus_a()
    lanes_seen = set()
    for w in ref.GAP_WIDTHS[1:]:
        docs = a.postings(ref.PF, "g%02d" % w)[0]
        gaps = np.diff(docs[:128])           # gap of posting j at index j-1
        top = np.nonzero(gaps >> (w - 1))[0] + 1
        assert (gaps < (1 << w)).all()
        segs = {int(j) // 32 for j in top}
        assert len(segs) == ref.WIDE_SEGS.get(w, 4), (w, segs)
        if w <= 13:   # the doc-id space allows all 127
            assert len(top) == 127
        else:
            lanes_seen.add(tuple(top.tolist()))
    assert len(lanes_seen) == 22 - 13
    for w in ref.TF_WIDTHS:
        for v in "nw":
            tf1 = a.postings(ref.PF, "f%02d%s" % (w, v))[1] - 1
            assert tf1.max() < (1 << w) and a.postings(
                ref.PF, "f%02d%s" % (w, v))[1].max() <= 1 << 20
            assert (tf1 >> (w - 1)).sum() >= 32


def test_block_counts_are_exactly_the_claimed_sets(real_a):
    for field, tfb in ((ref.PF, 2), (ref.PB, 0)):
        r = real_a[field]
        for n in ref.COUNTS:
            want = [128] * (n // 128) + ([n % 128] if n % 128 else [])
            narrow, wide = r["c%03dn" % n], r["c%03dw" % n]
            assert [b[2] for b in narrow] == want == [b[2] for b in wide]
            assert all(b[0] <= 3 for b in narrow)
            # a block of one posting has no gap to be wide
            assert all(b[0] == (17 if b[2] > 1 else 1) for b in wide), wide
        assert {b[2] for t, bl in r.items() if t[0] == "c" for b in bl} == \
            {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128}
        assert {sum(b[2] for b in bl) for t, bl in r.items()
                if t[0] == "c"} == set(ref.COUNTS)
        assert all(b[1] <= tfb for t, bl in r.items() if t[0] == "c"
                   for b in bl)


def test_tile_edge_and_pipeline_terms(real_a):
    a = ref.corpus_a()
    pf = real_a[ref.PF]
    T = ref.TILE_DOCS
    assert a.postings(ref.PF, "e0")[0].tolist() == \
        [0, T - 1, T, 2 * T - 1, ref.N_A - 1]
    assert pf["e0"] == [(22, 2, 5)]
    e1 = a.postings(ref.PF, "e1")[0]
    assert len(e1) == 128 and e1[0] < T <= e1[-1] and pf["e1"][0][2] == 128

    # p0: >= 24 blocks overlap one tile (three iterations per half-wave at
    # a stride of 8 blocks); consecutive blocks differ in both widths
    assert [b[0] for b in pf["p0"]] == ref.P0_ID_BITS
    assert [b[1] for b in pf["p0"]] == ref.P0_TF_BITS
    assert all(b[2] == 128 for b in pf["p0"])
    assert all(1 <= w <= 13 for b in pf["p0"] for w in b[:2])
    for x, y in zip(pf["p0"], pf["p0"][1:]):
        assert x[0] != y[0] and x[1] != y[1]
    lo = ref.P0_TILE * T
    br = ref.block_ranges(a.data, ref.PF, "p0")
    assert sum(1 for f, l in br if l >= lo and f < lo + T) == 26
    assert sum(1 for f, l in br if f >= lo and l < lo + T) >= 24
    assert br[0][0] < lo <= br[0][1]

    # p1: wide, eight dense, wide, all overlapping one tile
    assert [b[0] for b in pf["p1"]] == ref.P1_ID_BITS
    assert [b[1] for b in pf["p1"]] == ref.P1_TF_BITS
    lo = ref.P1_TILE * T
    br = ref.block_ranges(a.data, ref.PF, "p1")
    assert all(l >= lo and f < lo + T for f, l in br) and len(br) == 10
    docs = a.postings(ref.PF, "p1")[0]
    gaps = np.diff(docs)
    assert gaps[:128].max() >= 65536 and gaps[-127:].max() >= 65536
    assert br[0][0] < lo - 65536 and br[-1][1] >= lo + T + 57000
    # a block that spans hundreds of tiles
    f, l = ref.block_ranges(a.data, ref.PF, "g22")[0]
    assert l // T - f // T >= 256


def test_phrase_corpus_widths_and_counts(real_b):
    b = ref.corpus_b()
    assert b.num_docs == 200_000 and len(b.docs) < 2000
    n = len(ref.PAIR_SPECS)
    for k, (x, y) in enumerate(b.pairs):
        count, idw, tfw = ref.PAIR_SPECS[k % n]
        blocks = real_b[x if k < n else y]
        assert sum(bl[2] for bl in blocks) == count
        assert blocks[0][:2] == (idw, tfw), (k, blocks)
    for role in (0, 1):  # driver tokens, second tokens
        bl = [blk for p in b.pairs for blk in real_b[p[role]]]
        assert {x[0] for x in bl} == {1, 2, 3, 5, 8, 9, 12, 16, 17, 18}
        assert {x[1] for x in bl} >= {1, 3, 8, 9, 16, 17}
        assert {x[1] for x in bl} <= {1, 2, 3, 8, 9, 16, 17}
        assert {x[2] for x in bl} >= {1, 32, 33, 64, 65, 96, 97, 128}
        # exactly one doc of 65,537 repeats per role
        assert sum(x[1] == 17 for x in bl) == 1
    assert {sum(bl[2] for bl in real_b[t]) for p in b.pairs for t in p} >= \
        {1, 32, 33, 64, 65, 96, 97, 128, 129}
    assert max(int(np.diff(b.postings(t)[0]).max()) for p in b.pairs
               for t in p if len(b.postings(t)[0]) > 1) >= 1 << 17
    for x, y in b.pairs:
        h0, h1, h3 = (b.slop_hits([x, y], s) for s in ref.SLOPS)
        assert set(h0) <= set(h1) <= set(h3)
        both = [d for d in b.docs if {x, y} <= set(b.toks[d])]
        if len(both) >= 8:
            assert len(h0) < len(h1) < len(h3) < len(both)
            assert 2 * len(h0) >= len(both) - 8
        assert b.prefix_hits([x, y[:-1]]) == h0  # no other yNN follows x


# ------------------------------------------------ writer -> reader, no C++
def test_reader_returns_the_generators_arrays():
    a = ref.corpus_a()
    s = splitread.Split(a.data)
    for field in (ref.PF, ref.PB):
        assert s.terms(field) == sorted(a.terms[field])
        for t, (docs, tfs) in a.terms[field].items():
            d, f = s.postings(field, t)
            assert d.tolist() == docs.tolist(), (field, t)
            assert f.tolist() == tfs.tolist(), (field, t)
    b = ref.corpus_b()
    s = splitread.Split(b.data)
    assert s.terms("body") == b.vocab
    for t in b.vocab:
        docs, tfs = b.postings(t)
        d, f = s.postings("body", t)
        assert d.tolist() == docs.tolist() and f.tolist() == tfs.tolist(), t


def test_scores_of_one_term_are_separated_or_equal():
    a = ref.corpus_a()
    for field, t in ref.scored_terms():
        assert a.min_separation(field, t) >= ref.MIN_SEP, (field, t)
    s = np.unique([s for _, s in a.ranked(ref.PF, ["p0", "p1"])])
    assert (np.diff(s) / s[1:]).min() >= ref.MIN_SEP


# ------------------------------------------------- the oracle on the requests
_ORACLE = {}


def oracle(corpus):
    if corpus.split_id not in _ORACLE:
        s = OracleSearcher()
        s.add_split(corpus.split_id, corpus.data)
        _ORACLE[corpus.split_id] = s
    return _ORACLE[corpus.split_id]


def run(corpus, schema, query, kind, expected):
    req = make_leaf_request(
        query, schema, [(corpus.split_id, corpus.num_docs)],
        max_hits=len(expected) + (0 if kind == "scored" else 10),
        sort_fields=[{"field_name": "_score", "sort_order": 1}]
        if kind == "scored" else None)
    return oracle(corpus).leaf_search(req)


CASES_A = ref.cases_a()
CASES_B = [c for c in ref.cases_b() if c[0].endswith("slop0")]


@pytest.mark.parametrize("case", CASES_A, ids=[c[0] for c in CASES_A])
def test_oracle_matches_reference_on_widths_corpus(case):
    name, query, kind, expected = case
    # no case is empty but must: [a term of one posting] without that doc
    assert expected or name.startswith("must-") and "c001" in name, name
    resp = run(ref.corpus_a(), ref.SCHEMA_A, query, kind, expected)
    ref.check_response(resp, kind, expected, name)


@pytest.mark.parametrize("case", CASES_B, ids=[c[0] for c in CASES_B])
def test_oracle_matches_reference_on_phrase_corpus(case):
    name, query, kind, expected = case
    assert expected, name
    assert all(c[3] for c in ref.cases_b() + ref.cases_union())
    resp = run(ref.corpus_b(), ref.SCHEMA_B, query, kind, expected)
    ref.check_response(resp, kind, expected, name)
