"""Pure-Python reference for `terms(field) -> percentiles(field)`, computed
from the documents alone.

The sketch is the DDSketch restatement of csrc/qagg_format.h: relative
accuracy 0.01, gamma = 1.01 / 0.99, values below 1e-9 in a zero bucket, and
otherwise the key of v is the smallest k with v <= gamma^k. A percentile q
over n values reads the bucket whose cumulative count first exceeds
q * (n - 1) and reports 2 * gamma^k / (gamma + 1) (0.0 for the zero bucket).

Python's pow and the C library's may differ in the last bit of gamma^k, so a
value that sits on a bucket boundary could land on either side. sketch_key
therefore refuses (AssertionError) any value within 1e-9 relative of a
boundary: that is a condition on the test inputs, not on the engine.
"""
import math

ALPHA = 0.01
MIN_VALUE = 1e-9
GAMMA = (1.0 + ALPHA) / (1.0 - ALPHA)
DEFAULT_PERCENTS = [1, 5, 25, 50, 75, 95, 99]
BOUNDARY_GUARD = 1e-9

ZERO = None  # the zero bucket's key; sorts before every integer key


def sketch_key(v: float):
    """ZERO for v < 1e-9, else the smallest k with v <= GAMMA**k."""
    v = float(v)
    assert v >= 0.0, f"negative value {v!r}: the engine refuses these"
    if v < MIN_VALUE:
        assert abs(v - MIN_VALUE) > BOUNDARY_GUARD * MIN_VALUE, v
        return ZERO
    k = int(math.ceil(math.log(v) / math.log(GAMMA)))
    while GAMMA ** float(k) < v:
        k += 1
    while GAMMA ** float(k - 1) >= v:
        k -= 1
    for b in (GAMMA ** float(k), GAMMA ** float(k - 1)):
        assert abs(v - b) > BOUNDARY_GUARD * b, (
            f"value {v!r} within {BOUNDARY_GUARD} relative of boundary {b!r}")
    return k


def key_value(k) -> float:
    return 0.0 if k is ZERO else 2.0 * GAMMA ** float(k) / (GAMMA + 1.0)


def quantile(keys: list, q: float):
    """keys: one sketch key per value. None for an empty sketch."""
    n = len(keys)
    if n == 0:
        return None
    rank = q * float(n - 1)
    counts = {}
    for k in keys:
        counts[k] = counts.get(k, 0) + 1
    ordered = sorted(counts, key=lambda k: (k is not ZERO, k or 0))
    cum = 0
    for k in ordered:
        cum += counts[k]
        if float(cum) > rank:
            return key_value(k)
    return key_value(ordered[-1])


def percent_key(p) -> str:
    """The JSON key of a percent under `keyed: true`, as percentiles_to_json
    prints it at top level and under histograms: "50.0" for an integral
    percent, 17 significant digits otherwise."""
    p = float(p)
    return "%.1f" % p if p == math.floor(p) else "%.17g" % p


def percentiles(values: list, percents=None) -> dict:
    """{percent_key: value or None} over the non-null values."""
    keys = [sketch_key(v) for v in values if v is not None]
    return {percent_key(p): quantile(keys, p / 100.0)
            for p in (percents or DEFAULT_PERCENTS)}


def terms_percentiles(docs: list, terms_field: str, sub_field: str,
                      percents=None, match=None) -> dict:
    """{term: {"doc_count": n, "values": {percent_key: value or None}}} over
    the docs `match` accepts (all when None). A doc counts once per term
    value of `terms_field` (a str or a list of distinct strs) and adds its
    `sub_field` value, when it has one, to each of those terms' sketches."""
    groups = {}
    for d in docs:
        if match is not None and not match(d):
            continue
        t = d.get(terms_field)
        if t is None or t == "":
            continue
        for term in sorted(set([t] if isinstance(t, str) else t)):
            if term == "":
                continue
            g = groups.setdefault(term, {"doc_count": 0, "vals": []})
            g["doc_count"] += 1
            if d.get(sub_field) is not None:
                g["vals"].append(d[sub_field])
    return {t: {"doc_count": g["doc_count"],
                "values": percentiles(g["vals"], percents)}
            for t, g in groups.items()}


def shown_buckets(groups: dict, size: int, order=None) -> list:
    """Terms in the order a terms aggregation shows them: doc_count desc then
    key asc by default, or `order` = a sort key over (term, group); cut to
    `size`."""
    items = sorted(groups.items(),
                   key=order or (lambda kv: (-kv[1]["doc_count"], kv[0])))
    return items[:size]
