"""Corpora of the terms -> percentiles tests, shared by the CPU suite (which
checks every one against the reference's boundary guard) and the GPU suite.

Every corpus is a list of document dicts over SCHEMA. `svc` is the terms
column (also indexed raw, so `svc:T` is a term query), `tags` its multi-valued
sibling, `grp` a query-only field that splits the docs into a strict subset,
and lat / cnt / dl the f64 / u64 / i64 sub-aggregation columns.
"""
import math
import random

import numpy as np

from quickwit_amd import splitgen

TILE_DOCS = 8192

SCHEMA = {"timestamp_field": "ts", "fields": [
    {"name": "ts", "type": "datetime", "fast": True},
    {"name": "svc", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False, "fast": True},
    {"name": "tags", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False, "fast": True, "multi": True},
    {"name": "grp", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False},
    {"name": "lat", "type": "f64", "fast": True},
    {"name": "cnt", "type": "u64", "fast": True},
    {"name": "dl", "type": "i64", "fast": True},
]}

BULK_SCHEMA = {"timestamp_field": "ts", "fields": [
    {"name": "ts", "type": "datetime", "fast": True},
    {"name": "svc", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False, "fast": True},
    {"name": "grp", "type": "text", "tokenizer": "raw", "record": "basic",
     "fieldnorms": False},
    {"name": "lat", "type": "f64", "fast": True},
]}

Q_ALL = {"type": "match_all"}
Q_SUBSET = {"type": "term", "field": "grp", "value": "a"}
Q_NONE = {"type": "term", "field": "grp", "value": "zzz"}
TAGS = ["blue", "green", "red", "teal", "white", "yellow"]


def in_subset(d):
    return d["grp"] == "a"


def term_name(i, n_terms):
    return "s%0*d" % (len(str(n_terms - 1)), i)


def make_docs(n, seed, n_terms=5, p_null_svc=0.0, p_null_lat=0.0,
              lat=lambda rng: round(rng.uniform(0.5, 900.0), 3)):
    """Terms drawn with a skew (low ordinals are hot) so the top buckets are
    distinct by count; cnt and dl start at 2 (1 is the boundary gamma^0)."""
    rng = random.Random(seed)
    docs = []
    for i in range(n):
        d = {"ts": 1_700_000_000 + i,
             "grp": "a" if rng.random() < 0.4 else "b",
             "cnt": rng.randrange(2, 1_000_000),
             "dl": rng.randrange(2, 5_000)}
        if rng.random() >= p_null_svc:
            d["svc"] = term_name(int(n_terms * rng.random() ** 2), n_terms)
        d["tags"] = rng.sample(TAGS, rng.randrange(0, 4))
        if rng.random() >= p_null_lat:
            d["lat"] = lat(rng)
        docs.append(d)
    return docs


def wide_lat(rng):
    """1e-3 .. 1e9: about 1,400 sketch keys"""
    return float("%.9g" % math.exp(rng.uniform(math.log(1e-3), math.log(1e9))))


def decades_lat(lo, hi):
    def lat(rng):
        return float("%.9g" % math.exp(rng.uniform(math.log(lo), math.log(hi))))
    return lat


def zeroes_docs(n, seed):
    """values of 0 and below 1e-9 among ordinary ones, in every column"""
    docs = make_docs(n, seed, n_terms=4, lat=wide_lat)
    for i, d in enumerate(docs):
        if i % 7 == 0:
            d["lat"], d["cnt"], d["dl"] = 0.0, 0, 0
        elif i % 7 == 1:
            d["lat"] = 5e-10
    return docs


def all_null_bucket_docs(n, seed):
    """the bucket "nul" has members, none with a lat"""
    docs = make_docs(n, seed, n_terms=6, p_null_svc=0.2, p_null_lat=0.3)
    for i, d in enumerate(docs):
        if i % 5 == 0:
            d["svc"] = "nul"
            d.pop("lat", None)
    return docs


def segment_docs():
    """three segments whose dictionaries differ: each has terms of its own
    and shares some with the others"""
    segs = []
    for si in range(3):
        docs = make_docs(700 + 150 * si, 90 + si, n_terms=8)
        for i, d in enumerate(docs):
            if i % 4 == 0:
                d["svc"] = "only%d" % si
        segs.append(docs)
    return segs


def write_split(docs, split_id):
    w = splitgen.SplitWriter(SCHEMA, split_id, store_docs=False)
    w.add_documents(docs)
    return w.finalize()


BULK_CARD = 66_000
BULK_DOCS = 70_000


def bulk_corpus(seed=5):
    """66,000 terms on 70,000 docs, the 4,000
    spare docs on 20 hot terms with distinct counts. Returns (ords, grp, lat)
    arrays; bulk_docs() gives the dict form the reference reads."""
    rng = np.random.default_rng(seed)
    ords = np.arange(BULK_DOCS, dtype=np.int64)
    hot = rng.choice(BULK_CARD, size=20, replace=False)
    spare = BULK_DOCS - BULK_CARD
    weights = np.arange(20, 0, -1, dtype=np.float64)
    ords[BULK_CARD:] = rng.choice(hot, size=spare, p=weights / weights.sum())
    ords = rng.permutation(ords)
    grp = (rng.random(BULK_DOCS) < 0.4).astype(np.int64)  # 1 = "a"
    # 1e-3 .. 1e9, about 1,400 keys: 66,000 kept rows would pass 2^25 words
    lat = np.exp(rng.uniform(math.log(1e-3), math.log(1e9), BULK_DOCS))
    return ords, grp, lat


def bulk_docs(ords, grp, lat):
    return [{"svc": "t%05d" % o, "grp": "a" if g else "b", "lat": float(v)}
            for o, g, v in zip(ords.tolist(), grp.tolist(), lat.tolist())]


def bulk_split(ords, grp, lat, split_id):
    vocab = ["t%05d" % i for i in range(BULK_CARD)]
    gvocab = ["a", "b"]
    ts = (1_700_000_000_000 + np.arange(BULK_DOCS, dtype=np.int64) * 1000)
    return splitgen.build_split_from_columns(
        BULK_SCHEMA, split_id, BULK_DOCS,
        {"svc": ords.astype(np.int32)[:, None],
         "grp": (1 - grp).astype(np.int32)[:, None]},
        {"svc": vocab, "grp": gvocab},
        {"ts": (ts, None), "svc": (("ords", ords, vocab), None),
         "lat": (lat, None)})


def small_corpora():
    """name -> docs, for every corpus the GPU suite writes with SplitWriter"""
    out = {
        "one_doc": make_docs(1, 1),
        "tile_plus_37": make_docs(TILE_DOCS + 37, 2, n_terms=9),
        "width1": make_docs(3000, 3, n_terms=5),
        "width2": make_docs(3000, 4, n_terms=300),
        "nullable": make_docs(2500, 6, n_terms=6, p_null_svc=0.25,
                              p_null_lat=0.3),
        "all_null_bucket": all_null_bucket_docs(2500, 7),
        "zeroes": zeroes_docs(2100, 8),
        "wide": make_docs(9000, 9, n_terms=7, lat=wide_lat),
        # about 17,600 keys: the boundary table (138 KiB) stays in global
        # memory and so do the counters
        "huge": make_docs(1500, 12, n_terms=5, lat=decades_lat(1e-3, 1e150)),
        # about 4,950 keys under one term: the table (39 KiB) stays in global
        # memory, the single kept row (19 KiB of counters) goes to LDS
        "one_term": make_docs(1200, 13, n_terms=1,
                              lat=decades_lat(1e-3, 1e40)),
    }
    for si, docs in enumerate(segment_docs()):
        out["segment%d" % si] = docs
    return out
