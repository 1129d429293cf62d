"""terms -> percentiles, the parts that need no GPU: the pure-Python reference
against the existing top-level percentiles path (through the oracle), the
boundary guard over every test corpus, and the QAGG1 codec, key-merge and
finalize of terms results that carry sketches.
"""
import ctypes
import json
import os
import struct

import pytest

import terms_percentiles_corpora as corp
import terms_percentiles_reference as ref
from quickwit_amd import qagg
from quickwit_amd.api import OracleSearcher, make_leaf_request

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


class _Buf(ctypes.Structure):
    _fields_ = [("data", ctypes.POINTER(ctypes.c_uint8)),
                ("len", ctypes.c_size_t)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(os.path.join(REPO, "libquickwit_amd.so"))
    lib.qw_merge_intermediate_aggs.argtypes = [
        ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t),
        ctypes.c_size_t, ctypes.POINTER(_Buf)]
    lib.qw_finalize_agg_to_json.argtypes = [
        ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
        ctypes.POINTER(_Buf)]
    lib.qw_buf_free.argtypes = [ctypes.POINTER(_Buf)]
    return lib


def merge_blobs(lib, blobs):
    arr = (ctypes.c_char_p * len(blobs))(*blobs)
    lens = (ctypes.c_size_t * len(blobs))(*[len(b) for b in blobs])
    buf = _Buf()
    rc = lib.qw_merge_intermediate_aggs(arr, lens, len(blobs),
                                        ctypes.byref(buf))
    assert rc == 0
    out = ctypes.string_at(buf.data, buf.len)
    lib.qw_buf_free(ctypes.byref(buf))
    return out


def finalize(lib, blob, aggs):
    buf = _Buf()
    rc = lib.qw_finalize_agg_to_json(blob, len(blob),
                                     json.dumps(aggs).encode(),
                                     ctypes.byref(buf))
    assert rc == 0
    out = ctypes.string_at(buf.data, buf.len)
    lib.qw_buf_free(ctypes.byref(buf))
    return json.loads(out)


# ---- QAGG1 kind-3 blobs written and read by hand, from the layout comment
# of csrc/qagg_format.h. A sub payload is ("stats", (count, sum, min, max,
# sum_sq)) or ("sketch", zero, {key: count}).
def encode_terms_blob(name, subs, entries, matched, error_bound=0):
    """subs: [(sub name, sub_kind)]; entries: [(key, doc_count, [payload])]
    sorted by key."""
    o = bytearray(struct.pack("<IHH", qagg.MAGIC, qagg.VERSION, 1))
    o += struct.pack("<H", len(name)) + name.encode() + bytes([3])
    o += struct.pack("<H", len(subs))
    for sname, kind in subs:
        o += struct.pack("<H", len(sname)) + sname.encode() + bytes([kind])
    o += bytes([0]) + struct.pack("<QQI", matched, error_bound, len(entries))
    for key, dc, payloads in entries:
        o += struct.pack("<H", len(key)) + key.encode() + struct.pack("<Q", dc)
        for (_sn, kind), p in zip(subs, payloads):
            if kind == 1:
                assert p[0] == "sketch"
                o += struct.pack("<QI", p[1], len(p[2]))
                for k in sorted(p[2]):
                    o += struct.pack("<iQ", k, p[2][k])
            else:
                assert p[0] == "stats"
                o += struct.pack(qagg.STATS_FMT, *p[1])
    return bytes(o)


def decode_terms_blob(blob):
    magic, ver, n = struct.unpack_from("<IHH", blob, 0)
    assert (magic, ver, n) == (qagg.MAGIC, qagg.VERSION, 1)
    off = 8
    (nl,) = struct.unpack_from("<H", blob, off)
    name = blob[off + 2:off + 2 + nl].decode()
    off += 2 + nl
    assert blob[off] == 3
    (ns,) = struct.unpack_from("<H", blob, off + 1)
    off += 3
    subs = []
    for _ in range(ns):
        (sl,) = struct.unpack_from("<H", blob, off)
        subs.append((blob[off + 2:off + 2 + sl].decode(), blob[off + 2 + sl]))
        off += 3 + sl
    off += 1
    matched, err, ne = struct.unpack_from("<QQI", blob, off)
    off += 20
    entries = []
    for _ in range(ne):
        (kl,) = struct.unpack_from("<H", blob, off)
        key = blob[off + 2:off + 2 + kl].decode()
        (dc,) = struct.unpack_from("<Q", blob, off + 2 + kl)
        off += 10 + kl
        payloads = []
        for _sn, kind in subs:
            if kind == 1:
                zero, nk = struct.unpack_from("<QI", blob, off)
                off += 12
                counts = {}
                for _k in range(nk):
                    k, c = struct.unpack_from("<iQ", blob, off)
                    counts[k] = c
                    off += 12
                payloads.append(("sketch", zero, counts))
            else:
                payloads.append(
                    ("stats", struct.unpack_from(qagg.STATS_FMT, blob, off)))
                off += qagg.STATS_SIZE
        entries.append((key, dc, payloads))
    assert off == len(blob)
    return name, subs, entries, matched, err


SUBS = [("p", 1), ("st", 0), ("p2", 1)]


def _stats(vals):
    return ("stats", (len(vals), float(sum(vals)), float(min(vals)),
                      float(max(vals)), float(sum(v * v for v in vals))))


def _sketch(vals):
    zero, counts = 0, {}
    for v in vals:
        k = ref.sketch_key(v)
        if k is ref.ZERO:
            zero += 1
        else:
            counts[k] = counts.get(k, 0) + 1
    return ("sketch", zero, counts)


BLOB_A_VALUES = {"api": [3.5, 12.25, 12.3, 700.0, 0.0],
                 "etl": [44.0, 45.0],
                 "web": [2.5]}
BLOB_B_VALUES = {"api": [9.75, 1500.0],
                 "job": [0.25, 0.75, 2e-10],
                 "web": [2.5, 88.0]}


def _blob_of(values):
    entries = [(t, len(v), [_sketch(v), _stats(v), _sketch([x * 2 for x in v])])
               for t, v in sorted(values.items())]
    return encode_terms_blob("t", SUBS, entries,
                             sum(len(v) for v in values.values()))


AGGS = {"t": {"terms": {"field": "svc", "size": 10}, "aggs": {
    "p": {"percentiles": {"field": "lat"}},
    "st": {"stats": {"field": "lat"}},
    "p2": {"percentiles": {"field": "lat", "percents": [50, 99.9],
                           "keyed": False}}}}}


def test_codec_round_trip_with_sketches(lib):
    blob = _blob_of(BLOB_A_VALUES)
    assert merge_blobs(lib, [blob]) == blob  # qagg_format.h decode + encode
    entries = qagg.parse_blob(blob)          # qagg.py parse + serialize
    assert [(e.name, e.kind, e.sub_kinds) for e in entries] == [
        ("t", 3, [1, 0, 1])]
    assert qagg.serialize_blob(entries) == blob
    assert decode_terms_blob(blob)[2][0][2][0] == _sketch(BLOB_A_VALUES["api"])


def test_key_merge_overlapping_and_disjoint_terms(lib):
    merged = merge_blobs(lib, [_blob_of(BLOB_A_VALUES), _blob_of(BLOB_B_VALUES)])
    both = {}
    for vals in (BLOB_A_VALUES, BLOB_B_VALUES):
        for t, v in vals.items():
            both.setdefault(t, []).extend(v)
    name, subs, entries, matched, _err = decode_terms_blob(merged)
    assert (name, subs) == ("t", SUBS)
    assert matched == sum(len(v) for v in both.values())
    assert [e[0] for e in entries] == sorted(both)  # api etl job web
    for key, dc, payloads in entries:
        v = both[key]
        assert dc == len(v)
        assert payloads[0] == _sketch(v)
        assert payloads[2] == _sketch([x * 2 for x in v])
        assert payloads[1][1][0] == len(v)
        assert payloads[1][1][2:4] == (min(v), max(v))
    # merging in the other order gives the same blob
    assert merge_blobs(lib, [_blob_of(BLOB_B_VALUES),
                             _blob_of(BLOB_A_VALUES)]) == merged
    assert qagg.serialize_blob(qagg.parse_blob(merged)) == merged


def test_finalized_json_keyed_and_list(lib):
    j = finalize(lib, _blob_of(BLOB_A_VALUES), AGGS)
    buckets = {b["key"]: b for b in j["t"]["buckets"]}
    assert [b["key"] for b in j["t"]["buckets"]] == ["api", "etl", "web"]
    for t, v in BLOB_A_VALUES.items():
        b = buckets[t]
        assert b["doc_count"] == len(v)
        assert b["p"] == {"values": ref.percentiles(v)}  # keyed, default
        want2 = ref.percentiles([x * 2 for x in v], [50, 99.9])
        assert b["p2"] == {"values": [{"key": 50.0, "value": want2["50.0"]},
                                      {"key": 99.9, "value": want2[ref.percent_key(99.9)]}]}
        assert b["st"]["count"] == len(v)
    # an entry whose sketch is empty renders nulls, as under histograms
    empty = encode_terms_blob("t", SUBS, [
        ("api", 4, [("sketch", 0, {}), ("stats", (0, 0.0, 0.0, 0.0, 0.0)),
                    ("sketch", 0, {})])], 4)
    b = finalize(lib, empty, AGGS)["t"]["buckets"][0]
    assert b["p"] == {"values": {k: None for k in ref.percentiles([])}}
    assert b["p2"] == {"values": [{"key": 50.0, "value": None},
                                  {"key": 99.9, "value": None}]}


def test_blob_without_sketches_is_unchanged(lib):
    stats_only = encode_terms_blob(
        "t", [("st", 0), ("mx", 0)],
        [(t, len(v), [_stats(v), _stats(v)])
         for t, v in sorted(BLOB_A_VALUES.items())], 8, error_bound=2)
    assert merge_blobs(lib, [stats_only]) == stats_only
    assert qagg.serialize_blob(qagg.parse_blob(stats_only)) == stats_only
    no_subs = encode_terms_blob("t", [], [("api", 3, []), ("web", 1, [])], 4)
    assert merge_blobs(lib, [no_subs]) == no_subs
    # and one the engine's CPU restatement wrote: terms with stats subs
    docs = corp.make_docs(400, 11)
    s = OracleSearcher()
    s.add_split("c", corp.write_split(docs, "c"))
    aggs = {"t": {"terms": {"field": "svc", "size": 3}, "aggs": {
        "st": {"stats": {"field": "lat"}}}},
        "h": {"histogram": {"field": "cnt", "interval": 250000}, "aggs": {
            "p": {"percentiles": {"field": "lat"}}}}}
    resp = s.leaf_search(make_leaf_request(
        corp.Q_ALL, corp.SCHEMA, [("c", len(docs))], max_hits=0,
        aggregation=aggs))
    assert not resp.get("failed_splits")
    blob = resp["intermediate_aggregation_result"]
    assert merge_blobs(lib, [blob]) == blob
    assert qagg.serialize_blob(qagg.parse_blob(blob)) == blob


TRUNC_VALUES = {"a": [310.0, 290.0], "b": [3.5, 4.5, 5.5, 6.5, 7.5],
                "c": [90.0, 95.0, 97.0], "d": [20.0 + i for i in range(6)],
                "e": [700.0], "f": [40.0, 41.0, 42.0, 43.0]}


@pytest.fixture(scope="module")
def truncate_tool(tmp_path_factory):
    """tools/qagg_truncate_main.cpp: truncate_terms_split over a blob"""
    import subprocess
    exe = str(tmp_path_factory.mktemp("qagg") / "qagg_truncate")
    subprocess.run(["g++", "-std=c++17", "-O1",
                    os.path.join(REPO, "tools", "qagg_truncate_main.cpp"),
                    "-o", exe], check=True)

    def run(blob, *args):
        return subprocess.run([exe, *map(str, args)], input=blob,
                              stdout=subprocess.PIPE, check=True).stdout
    return run


@pytest.mark.parametrize("args,kept,error_bound", [
    ((3,), ["b", "d", "f"], 4),              # doc count desc: 6, 5, 4
    ((3, "_key", "asc"), ["a", "b", "c"], 0),
    ((3, "_key", "desc"), ["d", "e", "f"], 0),
    ((3, "st", "desc"), ["a", "c", "e"], 0),  # avg 300, 94, 700
    ((3, "st", "asc"), ["b", "d", "f"], 0),
    ((6,), ["a", "b", "c", "d", "e", "f"], 1),  # a full list, nothing cut
    ((9, "_key", "asc"), ["a", "b", "c", "d", "e", "f"], 0),
])
def test_truncation_keeps_each_sketch_with_its_term(truncate_tool, args, kept,
                                                    error_bound):
    blob = _blob_of(TRUNC_VALUES)
    _n, _s, before, matched, _e = decode_terms_blob(blob)
    by_key = {key: (dc, payloads) for key, dc, payloads in before}
    name, subs, after, matched2, err = decode_terms_blob(
        truncate_tool(blob, *args))
    assert (name, subs, matched2) == ("t", SUBS, matched)
    assert [e[0] for e in after] == kept
    assert err == error_bound
    for key, dc, payloads in after:
        assert (dc, payloads) == by_key[key], key
        assert payloads[0] == _sketch(TRUNC_VALUES[key])
        assert payloads[2] == _sketch([x * 2 for x in TRUNC_VALUES[key]])


def test_every_corpus_passes_the_boundary_guard():
    """sketch_key asserts that no input lies within 1e-9 relative of a bucket
    boundary; run it over every value the GPU suite sketches"""
    for name, docs in corp.small_corpora().items():
        for f in ("lat", "cnt", "dl"):
            for d in docs:
                if d.get(f) is not None:
                    ref.sketch_key(d[f])
    ords, grp, lat = corp.bulk_corpus()
    for v in lat.tolist():
        ref.sketch_key(v)
    with pytest.raises(AssertionError):
        ref.sketch_key(1.0)  # gamma^0
    with pytest.raises(AssertionError):
        ref.sketch_key(ref.GAMMA ** 17.0)


@pytest.mark.parametrize("corpus,field", [
    ("width1", "lat"), ("nullable", "lat"), ("zeroes", "lat"),
    ("zeroes", "cnt"), ("zeroes", "dl"), ("wide", "lat")])
def test_reference_equals_top_level_percentiles(corpus, field):
    """For each term T the reference's bucket equals the oracle's answer to a
    top-level percentiles under `query AND svc:T`."""
    docs = corp.small_corpora()[corpus]
    s = OracleSearcher()
    s.add_split("c", corp.write_split(docs, "c"))
    percents = [1, 25, 50, 75, 95, 99.9]
    groups = ref.terms_percentiles(docs, "svc", field, percents,
                                   match=corp.in_subset)
    assert len(groups) >= 3
    aggs = {"p": {"percentiles": {"field": field, "percents": percents}}}
    for term, g in groups.items():
        q = {"type": "bool", "must": [
            corp.Q_SUBSET, {"type": "term", "field": "svc", "value": term}]}
        resp = s.leaf_search(make_leaf_request(
            q, corp.SCHEMA, [("c", len(docs))], max_hits=0, aggregation=aggs))
        assert not resp.get("failed_splits"), resp.get("failed_splits")
        assert resp.get("num_hits", 0) == g["doc_count"]
        j = s.finalize_agg_json(resp["intermediate_aggregation_result"], aggs)
        assert j["p"]["values"] == g["values"], term
