#!/usr/bin/env python3
"""Flagship benchmark: Quickwit leaf-search hot path on MI355X.

Default workload — THE HEADLINE CONFIG BASELINE.json's metric is quoted on
("3-term BM25 over 100M docs"): 3-term BM25 disjunction (OR) over 100M
synthetic log docs (hdfs-logs schema, seeded generator — SURVEY.md §8d), 1
split per GPU, max_hits=10, sorted by _score desc. It fits one GPU (~3.6 GB
split in 288 GB HBM). A "step" is one full leaf_search call over the split
batch, inputs already resident in HBM (the reference's warm state that
cpu_search_microsecs times, leaf.rs:905-946) + the cross-rank merge when
N>1. configs[1] (10M docs) is reachable with --docs 10000000.

Contract: python bench.py --gpus N --steps K --warmup W
  N>1 is launched by the driver via torch.distributed.run, one rank per GPU
  over RCCL; splits shard one-batch-per-GPU ("scaling": "weak");
  the only exchange is the packed-tensor merge (merge.distributed_merge:
  32 B top-K records allgather + dense-bucket sum-reduce + sideband bytes,
  no pickled objects).
Rank 0 prints ONE JSON line with metric/value/ms_per_step. A plain run does
only what that headline needs: set up, warm up, time the K steps, write the
outputs when --dump-outputs is given, print the line (roofline and
cpu_baseline are null). --full adds the secondary measurements:
  roofline: dominant kernel algorithmic-bytes/launch over its HIP-event
    launch time, vs 8 TB/s HBM3E peak (MI355X_MICROARCH.md). Algorithmic
    bytes are counted from the generated index, not from DRAM
    traffic. traffic stays null here; PMC evidence lives under profiles/.
  cpu_baseline: the oracle (reference restatement, kind "port") timed on this
    box's host cores on a bounded sample (--cpu-baseline-docs), repeated
    until >=2 s of wall time so the rate is honestly measurable.

--dump-outputs DIR writes what the last timed step returned (the decoded
LeafSearchResponse a caller receives: counts, top-K hits, finalized
aggregations) as DIR/<name>.npy float64 arrays, all finite: an optional
value comes with a <name>_state array (1 value, 0 absent). Inputs are
seeded, so two builds run with the same arguments can be compared output
for output.

Extra workloads (NOT the default the driver runs):
  --workload range    bool must severity_text:INFO + u64 tenant_id range
  --workload agg      date_histogram(1h) + terms(tenant) under match_all
                      (--splits 8 = config #4's per-GPU shape)
  --workload config5  top-1000 BM25 + range filter + terms agg
                      (--docs 125000000 --splits 8 = configs[4]'s 1-GPU slice)
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
TILE_DOCS = 8192

BM25_TERMS = ["w%05d" % i for i in (9, 10, 11)]
# Zipf ranks 10-12: P(doc contains term) = 1-(1-p_r)^10 ≈ 10% each, matching
# SURVEY §8d config 2 ("chosen at df≈10% each"); the top ranks sit at ≈66%.

AGGS = {"per_hour": {"date_histogram": {"field": "timestamp",
                                        "fixed_interval": "3600000ms"}},
        "per_tenant": {"terms": {"field": "tenant_name", "size": 10}}}


def _doc_freq(sp, field, term):
    tid = sp.term_id(field, term)
    return 0 if tid is None else int(sp._sec(field, "doc_freq", "<u4")[tid])


def _posting_bytes(sp, field, term, n_tiles):
    posting_off = sp._sec(field, "posting_off", "<u8")
    n_blocks = sp._sec(field, "n_blocks", "<u4")
    tid = sp.term_id(field, term)
    if tid is None:
        return 0
    return (int(posting_off[tid + 1] - posting_off[tid]) +
            int(n_blocks[tid]) * 16 + 2 * 4 * n_tiles)


def make_workload(name, docs, max_hits):
    """-> dict(query, sort, aggregation, max_hits, kernel, algo_bytes(fn),
    label, query_str)."""
    if name == "bm25":
        return {
            "query": {"type": "bool", "should": [
                {"type": "term", "field": "body", "value": t}
                for t in BM25_TERMS]},
            "sort": [{"field_name": "_score", "sort_order": 1}],
            "aggregation": None, "max_hits": max_hits,
            "kernel": "union_bm25",
            "label": f"3term_bm25_or_{docs}",
            "query_str": " OR ".join(f"body:{t}" for t in BM25_TERMS),
            # postings+skip+ranges of 3 terms + 1B fieldnorm + 8B candidate
            # record per union hit + tile counts
            "algo_bytes": lambda sp, nh, nt: (
                sum(_posting_bytes(sp, "body", t, nt) for t in BM25_TERMS)
                + nh * (1 + 8) + nt * 4),
        }
    if name == "range":
        q = {"type": "bool",
             "must": [{"type": "term", "field": "severity_text",
                       "value": "INFO"}],
             "filter": [{"type": "range", "field": "tenant_id",
                         "lower_bound": {"included": 100},
                         "upper_bound": {"excluded": 300}}]}
        return {
            "query": q, "sort": None, "aggregation": None,
            "max_hits": max_hits, "kernel": "union_bm25",
            "label": f"must_info_tenant_range_{docs}",
            "query_str": "severity_text:INFO AND tenant_id:[100..300)",
            # must postings + 8B u64 column gather per INFO doc (the pred is
            # evaluated on must-matched docs only); the INFO doc count is
            # read from the index (doc_freq), not assumed
            "algo_bytes": lambda sp, nh, nt: (
                _posting_bytes(sp, "severity_text", "INFO", nt)
                + _doc_freq(sp, "severity_text", "INFO") * 8
                + nh * 8 + nt * 4),
        }
    if name == "agg":
        return {
            "query": {"type": "match_all"}, "sort": None,
            "aggregation": AGGS, "max_hits": 0,
            "kernel": "column_agg",
            "label": f"datehisto_terms_agg_{docs}",
            "query_str": "* with per_hour date_histogram + per_tenant terms",
            # 8B ts + 2B tenant ord per doc. The per-workgroup LDS flush
            # (<=2048 WGs x (720+1000) u64 slots ~ 28 MB, ~3%) is counted as
            # overhead, not algorithmic bytes — PMC FETCH+WRITE in
            # profiles/ corroborates total traffic ~= these bytes + flush.
            "algo_bytes": lambda sp, nh, nt: nt * TILE_DOCS * (8 + 2),
        }
    if name == "config5":
        # BASELINE.json configs[4]: top-1000 BM25 + fast-field filter +
        # terms agg (the 8-GPU slice is 1B docs / 64 splits; the 1-GPU slice
        # is --docs 125000000 --splits 8 = 8 x 15.6M-doc splits)
        q = {"type": "bool",
             "should": [{"type": "term", "field": "body", "value": t}
                        for t in BM25_TERMS],
             "filter": [{"type": "range", "field": "tenant_id",
                         "lower_bound": {"included": 100},
                         "upper_bound": {"excluded": 900}}]}

        def _algo(sp, nh, nt):
            # postings of the 3 should terms + 8B tenant gather per
            # union-matched doc (union size analytic from the per-term
            # df under the generator's independence) + 1B norm + 16B wide
            # candidate record per post-filter hit + tile counts
            nd = nt * TILE_DOCS
            prod = 1.0
            for t in BM25_TERMS:
                prod *= 1.0 - _doc_freq(sp, "body", t) / nd
            union = int(nd * (1.0 - prod))
            return (sum(_posting_bytes(sp, "body", t, nt) for t in BM25_TERMS)
                    + union * (8 + 1) + nh * 16 + nt * 4)
        return {
            "query": q,
            "sort": [{"field_name": "_score", "sort_order": 1}],
            "aggregation": {"per_tenant": {"terms": {"field": "tenant_name",
                                                     "size": 10}}},
            "max_hits": 1000, "kernel": "union_bm25",
            "label": f"top1000_bm25_filter_terms_{docs}",
            "query_str": "3-term OR, tenant_id:[100..900), top-1000, terms agg",
            "algo_bytes": _algo,
        }
    raise SystemExit(f"unknown workload {name}")


def cached_split(rank, docs, seed=42):
    from quickwit_amd import splitgen
    path = os.path.join(tempfile.gettempdir(),
                        f"qwa1-{seed}-{rank}-{docs}.bin")
    if os.path.exists(path) and os.path.getsize(path) > 0:
        with open(path, "rb") as f:
            return f.read()
    data = splitgen.generate_split(rank, docs, seed=seed)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            f.write(data)
        os.rename(tmp, path)
    except OSError:
        pass
    return data


def _finite(x):
    """-> (value, state). Every dumped number is finite: a value the response
    does not carry (state 0) or a non-finite one (2 nan, 3 +inf, 4 -inf) is
    written as 0.0 and told apart by its state; 1 = ordinary value."""
    if x is None:
        return 0.0, 0.0
    x = float(x)
    if math.isfinite(x):
        return x, 1.0
    return 0.0, 2.0 if math.isnan(x) else 3.0 if x > 0 else 4.0


def _sort_value(sv):
    """SortByValue oneof -> number (None when the hit carries none)."""
    for k in ("f64", "u64", "i64", "boolean"):
        if sv and k in sv:
            return sv[k]
    return None


def _flatten_numbers(node, out):
    """Leaves of a finalized aggregation JSON in a fixed order (dict keys
    sorted, lists in order); string keys enter as their CRC32 so bucket
    identity is compared too, null metrics stay null."""
    if isinstance(node, dict):
        for k in sorted(node):
            _flatten_numbers(node[k], out)
    elif isinstance(node, list):
        for v in node:
            _flatten_numbers(v, out)
    elif isinstance(node, str):
        out.append(zlib.crc32(node.encode()))
    else:
        out.append(node)


def dump_outputs(out_dir, resp, searcher, aggregation):
    """Write the last timed step's response as float64 .npy arrays (a few KB:
    top-K hits and finalized buckets, never per-doc data). Timings
    (resource_stats) are not outputs and stay out. Optional values come as
    a <name> / <name>_state pair (_finite)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    hits = resp.get("partial_hits", [])
    arrays = {
        "counts": [resp.get("num_hits", 0),
                   resp.get("num_attempted_splits", 0),
                   resp.get("num_successful_splits", 0),
                   len(resp.get("failed_splits", []))],
        "hit_doc_id": [h.get("doc_id", 0) for h in hits],
        "hit_segment_ord": [h.get("segment_ord", 0) for h in hits],
        # split ids are synthetic-<seed>-<ordinal>
        "hit_split_ord": [int(h["split_id"].rsplit("-", 1)[1]) for h in hits],
    }
    optional = {
        "hit_sort_value": [_sort_value(h.get("sort_value")) for h in hits],
        "hit_sort_value2": [_sort_value(h.get("sort_value2")) for h in hits],
    }
    blob = resp.get("intermediate_aggregation_result")
    if aggregation and blob:
        flat = []
        _flatten_numbers(searcher.finalize_agg_json(blob, aggregation), flat)
        optional["agg_values"] = flat
    for name, vals in optional.items():
        pairs = [_finite(v) for v in vals]
        arrays[name] = [v for v, _ in pairs]
        arrays[name + "_state"] = [st for _, st in pairs]
    for name, vals in arrays.items():
        arr = np.asarray(vals, dtype=np.float64)
        if arr.size == 0:
            continue  # no hits requested: counts.npy already says so
        assert np.isfinite(arr).all(), name
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--docs", type=int, default=100_000_000,
                    help="docs per split (one split per GPU); 100M is the "
                         "headline config of BASELINE.json's metric")
    ap.add_argument("--max-hits", type=int, default=10)
    ap.add_argument("--workload", default="bm25",
                    choices=["bm25", "range", "agg", "config5"])
    ap.add_argument("--splits", type=int, default=1,
                    help="splits per GPU (docs are divided across them); "
                         "config5's 1-GPU slice is --docs 125000000 "
                         "--splits 8")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as "
                         "DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also compute the roofline figure and time the CPU "
                         "baseline (off by default: a plain run measures "
                         "the headline only)")
    ap.add_argument("--cpu-baseline-steps", type=int, default=2)
    ap.add_argument("--cpu-baseline-docs", type=int, default=0,
                    help="oracle sample size (0 = min(docs, 10M))")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world > 1 and "QW_GEN_THREADS" not in os.environ:
        # torchrun defaults workers to OMP_NUM_THREADS=1, which would make
        # each rank's native split generation single-threaded (minutes at
        # 100M docs); give each rank an explicit share of the host cores
        # (qw_gen_set_threads overrides the OpenMP env pin)
        os.environ["QW_GEN_THREADS"] = str(
            max(1, (os.cpu_count() or 8) // world))

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        dist.init_process_group(backend)
        if torch.cuda.is_available():
            torch.cuda.set_device(local_rank)

    from quickwit_amd import proto, splitgen, splitread
    from quickwit_amd.api import GpuSearcher, OracleSearcher, make_leaf_request
    from quickwit_amd.merge import distributed_merge

    # QW_BENCH_ENGINE=oracle: CPU-only dry run of the FULL bench path (incl.
    # the N>1 packed exchange over gloo) for tests — never the measured
    # engine (tests/test_bench_distributed.py); the product run requires
    # the GPU and fails loudly without one.
    engine = os.environ.get("QW_BENCH_ENGINE", "gpu")

    wl = make_workload(args.workload, args.docs, args.max_hits)

    t_gen = time.perf_counter()
    docs_per_split = args.docs // args.splits
    searcher = (OracleSearcher() if engine == "oracle"
                else GpuSearcher(device=local_rank))
    split_set = []
    split_bytes = None
    for si in range(args.splits):
        ordn = rank * 64 + si
        data = cached_split(ordn, docs_per_split)
        if split_bytes is None:
            split_bytes = data  # algo-bytes accounting reads split 0
        sid = f"synthetic-42-{ordn:04d}"
        searcher.add_split(sid, data)
        split_set.append((sid, docs_per_split))
    sid = split_set[0][0]
    gen_s = time.perf_counter() - t_gen

    req = make_leaf_request(
        wl["query"], splitgen.HDFS_SCHEMA, split_set,
        max_hits=wl["max_hits"], sort_fields=wl["sort"],
        aggregation=wl["aggregation"])
    req_pb = proto.encode("LeafSearchRequest", req)
    sreq_pb = proto.encode("SearchRequest", req["search_request"])

    def one_step():
        resp_pb = searcher.leaf_search_raw(req_pb)
        if world > 1:
            # packed-tensor exchange over RCCL/xGMI: 32B hit
            # records allgather + dense-bucket sum-reduce + sideband bytes
            merged = distributed_merge(sreq_pb, resp_pb,
                                       [s for s, _ in split_set])
            return merged if rank == 0 else resp_pb
        return resp_pb

    for _ in range(args.warmup):
        last = one_step()
    if engine != "oracle":
        searcher.kernel_stats_reset()

    if dist:
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    step_times = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        last = one_step()
        step_times.append(time.perf_counter() - ts)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.barrier()

    if rank != 0:
        return

    resp = proto.decode("LeafSearchResponse", last)
    num_hits = resp.get("num_hits", 0)
    per_split_hits = num_hits // world if world > 1 else num_hits
    total_docs = args.docs * world
    value = args.steps * total_docs / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    p50_ms = sorted(step_times)[len(step_times) // 2] * 1e3

    if args.dump_outputs:
        dump_outputs(args.dump_outputs, resp, searcher, wl["aggregation"])

    # roofline of the dominant kernel (--full)
    kms, launches = (searcher.kernel_stats(wl["kernel"])
                     if args.full and engine != "oracle" else (0.0, 0))
    roofline = None
    if launches:
        ms_per_launch = kms / launches
        n_tiles = (docs_per_split + TILE_DOCS - 1) // TILE_DOCS
        sp = splitread.Split(split_bytes)
        ab = int(wl["algo_bytes"](sp, per_split_hits // args.splits, n_tiles))
        achieved = ab / (ms_per_launch / 1e3) / 1e9
        roofline = {"bound": "hbm", "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": None,  # PMC evidence committed under profiles/
                    "kernel": wl["kernel"],
                    "algo_bytes_per_launch": ab,
                    "ms_per_launch": round(ms_per_launch, 4)}

    # CPU baseline: the oracle restatement (kind "port") on ALL host cores
    # (SURVEY §8d): the reference's rayon model is one thread per split, so
    # the sample is sharded into nproc splits and the oracle's OpenMP loop
    # runs one split per core. Bounded sample so the default run finishes in
    # minutes. (--full)
    cpu_baseline = None
    if args.full and world == 1 and args.cpu_baseline_steps > 0:
        ncores = os.cpu_count() or 1
        bdocs = args.cpu_baseline_docs or min(args.docs, 10_000_000)
        per = max(bdocs // ncores, 1)
        cpu = OracleSearcher()
        bsplits = []
        for i in range(ncores):
            sid = f"cpu-42-{i:04d}"
            cpu.add_split(sid, cached_split(1000 + i, per))
            bsplits.append((sid, per))
        breq = make_leaf_request(
            wl["query"], splitgen.HDFS_SCHEMA, bsplits,
            max_hits=wl["max_hits"], sort_fields=wl["sort"],
            aggregation=wl["aggregation"])
        breq_pb = proto.encode("LeafSearchRequest", breq)
        cpu.leaf_search_raw(breq_pb)  # warm
        # repeat until >=2 s of wall time so the rate is honestly timed (a
        # single call on many cores can finish in ~50 ms)
        calls = 0
        tc = time.perf_counter()
        elapsed_cpu = 0.0
        while calls < args.cpu_baseline_steps or elapsed_cpu < 2.0:
            cpu.leaf_search_raw(breq_pb)
            calls += 1
            elapsed_cpu = time.perf_counter() - tc
            if calls >= 200:
                break
        tcpu = elapsed_cpu / calls
        cpu_baseline = {
            "value": round(per * ncores * calls / elapsed_cpu, 1),
            "unit": "docs/s",
            "cores": ncores, "kind": "port",
            "sample": f"{calls} leaf_search calls over {ncores} splits x "
                      f"{per} docs, one OpenMP thread per split "
                      f"({tcpu * 1e3:.1f} ms each, {elapsed_cpu:.2f}s total)"}

    out = {
        "metric": "leaf_search_docs_per_sec",
        "value": round(value, 1),
        "unit": "docs/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "p50_ms": round(p50_ms, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,  # no published leaf-search number
        "dtype": "u32+f32",
        "data": "synthetic",
        "config": {
            "workload": wl["label"],
            "query": wl["query_str"],
            "docs_per_gpu": docs_per_split * args.splits,
            "splits_per_gpu": args.splits,
            "max_hits": wl["max_hits"],
            "num_hits_per_split": per_split_hits,
            "parallelism": f"split-dp{world}",
            "gen_seconds": round(gen_s, 1),
            "hbm_used_gb": (round(searcher.memory_stats()[0] / 2**30, 2)
                            if engine != "oracle" else None),
            "hbm_budget_gb": (round(searcher.memory_stats()[1] / 2**30, 1)
                              if engine != "oracle" else None),
        },
        "roofline": roofline,
        "cpu_baseline": cpu_baseline,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
