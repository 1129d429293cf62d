"""The HIP leaf path against the exact float64 reference of
tests/topk_reference.py: candidate emission, key encoding, the histogram
select and the host rebuild of hits, id-exact at the cut.

test_topk_reference_cpu.py has already proved the reference against the
oracle; nothing here reads the oracle. Scores are compared at the project's
1e-5 (REL of the other GPU tests, not re-derived); everything else — doc ids,
num_hits, column values, the sign of an f64 zero — is compared exactly, and
no hit or tie group is exempt.

DETERMINED cases (at most two scoring terms, and every field sort): the
returned list of (doc_id, sort_value, sort_value2) must equal the
reference's. ORDER-DEPENDENT cases (three and five should-terms) get the
weaker property checks of test_order_dependent; see its docstring.

Why each case reaches its path. The constants are product.cpp's; if they
change, the arithmetic below stops holding and must be redone, or a case
turns vacuous without failing.

  rerun_select refines (one 12-bit histogram pass per loop, at most four:
  prefix_bits < 48) while  survivors > max(4*K, 16384),  K = max_hits +
  start_offset (+1024 under search_after).

  Narrow records (one-field _score sort): key = f32-sortable score << 32 |
  doc, both halves complemented when ascending. The tied corpus has 70,000
  candidates with ONE score, so they share the upper 32 key bits; doc ids are
  below 2^17, so bits 31..17 are shared too.
    K = 1, 10, 4096, 4097: 70,000 > 16,384 (and > 4*4097). Passes 1-3 see
      one bin (more than 16,384 candidates share 12, 24 and 36 bits). Pass 4
      covers key bits 27..16 and splits on doc bit 16: descending, docs
      >= 65,536 (4,464 of them) fill the upper bin, which holds K, so 4,464
      survive; ascending the upper bin is the 65,536 docs below 65,536.
    K = 16384, 16385: 4*K = 65,536 / 65,540 < 70,000, the 4*K arm of the
      threshold. Descending, K exceeds the 4,464-doc upper bin of pass 4, so
      the walk crosses a bin edge and all 70,000 survive to the host sort.
    K = 70,000: no pass at all.
    start_offset 5,000 + max_hits 10: K = 5,010 > 4,464, crosses the bin.
  Class corpora: the 17,000- and 30,000-doc classes each keep one score, so
  a cut inside them runs all four passes the same way.

  Wide records (field sorts and two-field sorts): key = the monotonic u64 of
  the primary value, 0 when missing, complemented when ascending. u64 0
  (descending) and u64 max (ascending) therefore share key 0 with a missing
  value; so do i64 min / i64 max. The host re-sort must put the real value
  first; max_hits = U_CUM[order][3] +- 1 (22,199 .. 22,201) and I_CUM
  (259 .. 261) cut inside that collision. All cuts are below 17,500, so
  70,000 > max(4*K, 16384) holds: four passes, then 47,800 + 5,000 (or
  + 100) candidates with key 0 survive together.

  search_after retries with sel_kwant * 8 while the page is short, starting
  from sel_kwant = max_hits + 1024 = 1,524. A cursor at rank r of a tie group
  leaves r ties sorting before it. r = 20,000: 1,524 -> 12,192 (< 20,501)
  -> 97,536, capped at the band: two retries. r = 1,500 stays within the
  first selection's survivors; r = 0 is the plain case.

  Edge sweep: TILE_DOCS = 8192, posting blocks of 128, null words of 64 bits.
"""
import numpy as np
import pytest

import topk_reference as ref
from quickwit_amd.api import GpuSearcher, make_leaf_request

pytestmark = pytest.mark.gpu

# largest relative deviation of a GPU score from s64 over the module
DEVIATION = {"max": 0.0, "scores": 0}


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


class Gpu:
    """One device context; each corpus's split is built and uploaded once."""

    def __init__(self):
        self.searcher = GpuSearcher(device=0)
        self.loaded = set()

    def run(self, c, q, sort, max_hits, start_offset=0, after=None):
        if c.split_id not in self.loaded:
            self.searcher.add_split(c.split_id, c.data)
            self.loaded.add(c.split_id)
        req = make_leaf_request(
            q.ast(), ref.SCHEMA, [(c.split_id, c.num_docs)], max_hits=max_hits,
            start_offset=start_offset,
            sort_fields=ref.sort_fields(sort) or None)
        if after is not None:
            req["search_request"]["search_after"] = after
        try:
            resp = self.searcher.leaf_search(req)
        except RuntimeError as e:
            # a device error is not a mismatch: start nothing more on the GPU
            pytest.exit(f"leaf_search failed, stopping the run: {e}", 3)
        return ref.hits_of(resp)


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


def check_exact(got, exp, sort, what):
    dev = ref.assert_hits_exact(got, exp, sort, what)
    DEVIATION["max"] = max(DEVIATION["max"], dev)
    DEVIATION["scores"] += sum(len(got[1]) for f, _ in sort if f == "_score")


DETERMINED = [(name, corpus, q, sort, k)
              for name, corpus, q, sort, ks in ref.determined_cases()
              for k in ks]


@pytest.mark.parametrize("case", DETERMINED,
                         ids=[f"{c[0]}-k{c[4]}" for c in DETERMINED])
def test_determined(gpu, case):
    name, corpus, q, sort, k = case
    c = corpus()
    got = gpu.run(c, q, sort, k)
    check_exact(got, ref.expected(c, q, sort, k), sort, (name, k))
    if name.startswith("tied-score"):
        assert len({s for _, s, _ in got[1]}) == 1, "tied scores differ in bits"


@pytest.mark.parametrize("sort", [ref.SCORE_DESC, ref.SCORE_ASC],
                         ids=["desc", "asc"])
def test_tied_start_offset(gpu, sort):
    c = ref.tied_corpus()
    got = gpu.run(c, ref.AA, sort, 10, start_offset=5_000)
    check_exact(got, ref.expected(c, ref.AA, sort, 10, start_offset=5_000),
                sort, "start_offset")
    assert len({s for _, s, _ in got[1]}) == 1


AFTER = [(case, r) for case in ref.AFTER_CASES for r in ref.AFTER_RANKS]


@pytest.mark.parametrize("case,r", AFTER,
                         ids=[f"{c[0]}-rank{r}" for c, r in AFTER])
def test_search_after_through_tie_group(gpu, case, r):
    name, corpus, q, sort = case
    c = corpus()
    n, full = ref.ranked(c, q, sort)
    field = sort[0][0]
    # a score cursor carries the engine's own f32 value, as a client's would;
    # the tied corpus has one score, so a one-hit response supplies it
    score = gpu.run(c, q, sort, 1)[1][0][1] if field == "_score" else None
    cur = ref.cursor_of(c, full[r], field, score=score)
    got = gpu.run(c, q, sort, ref.AFTER_PAGE, after=cur)
    check_exact(got, (n, full[r + 1:r + 1 + ref.AFTER_PAGE]), sort, (name, r))
    # value-only cursor (no doc address): skips the cursor's whole tie group
    cur = ref.cursor_of(c, full[r], field, with_doc=False, score=score)
    rest = [h for h in full[r + 1:] if h[1] != full[r][1]]
    got = gpu.run(c, q, sort, ref.AFTER_PAGE, after=cur)
    check_exact(got, (n, rest[:ref.AFTER_PAGE]), sort, (name, r, "value-only"))


@pytest.mark.parametrize("n", ref.EDGE_SIZES)
def test_edge_sweep(gpu, n):
    c = ref.edge_corpus(n)
    for name, q, sort, k in ref.edge_queries(n):
        check_exact(gpu.run(c, q, sort, k), ref.expected(c, q, sort, k), sort,
                    (n, name))


def _order_dependent_cases():
    c = ref.classes_corpus()
    out = []
    for name, q in ref.ORDER_DEPENDENT:
        desc = ref.class_cums(c, q)
        asc = ref.class_cums(c, q, ref.ASC)
        out += [(name, q, ref.SCORE_DESC, k)
                for k in [10, desc[0] // 2] + ref.around(desc[:4])]
        out += [(name, q, ref.SCORE_ASC, k)
                for k in [10] + ref.around(asc[:2])]
    return out


ORDER_DEPENDENT = _order_dependent_cases()


@pytest.mark.parametrize(
    "case", ORDER_DEPENDENT,
    ids=[f"{n}-{'desc' if s[0][1] else 'asc'}-k{k}"
         for n, _, s, k in ORDER_DEPENDENT])
def test_order_dependent(gpu, case):
    """Scored queries of three and five should-terms. These checks are weaker
    than list equality, and that is a property of the kernel, not of the
    test: should-terms accumulate into the LDS score tile with atomicAdd and
    no barrier between terms, so an f32 sum of three or more terms depends on
    arrival order. Two docs with identical inputs may differ in the last bit,
    and one run may order them differently from the next. What is fixed:
    the match count; every score to 1e-5 of s64; the list is sorted by what
    it returns; every class wholly above the cut comes back as its exact id
    set (classes are 1e-3 apart, 100 tolerances); the cut class contributes
    exactly its share, from its own members; nothing left out beats the last
    hit by more than the tolerance."""
    name, q, sort, k = case
    c = ref.classes_corpus()
    desc = sort[0][1] == ref.DESC
    n, full = ref.ranked(c, q, sort)
    num_hits, hits = gpu.run(c, q, sort, k)
    assert num_hits == n
    assert len(hits) == min(k, n)
    s64 = ref.scores64(c, q)
    ids = [d for d, _, _ in hits]
    assert len(set(ids)) == len(ids)
    for d, s, _ in hits:
        dev = abs(s - s64[d]) / s64[d]
        DEVIATION["max"] = max(DEVIATION["max"], dev)
        assert dev <= ref.REL, (d, s, s64[d])
    DEVIATION["scores"] += len(hits)
    # strictly ordered by (returned score, doc id), both in the sort direction
    for (da, sa, _), (db, sb, _) in zip(hits, hits[1:]):
        before = (sa, da) > (sb, db) if desc else (sa, da) < (sb, db)
        assert before, ((da, sa), (db, sb))
    # classes in rank order; the reference's top-k fixes each class's share
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
        if share == len(members[s]):  # wholly above the cut: exact id set
            assert got_by_class[s] == members[s], ("class", s)
        else:  # the cut class: exactly its share (its members by the key)
            assert len(got_by_class[s]) == share, ("cut class", s)
    # no unreturned doc beats the last returned score beyond the tolerance
    left = np.ones(c.num_docs, dtype=bool)
    left[ids] = False
    left &= ref.match_mask(c, q)
    last = hits[-1][1]
    if desc:
        assert not (s64[left] * (1 - ref.REL) > last).any()
    else:
        assert not (s64[left] * (1 + ref.REL) < last).any()


def test_zz_score_deviation_report():
    """Runs last in the module: the largest relative deviation of any GPU
    score from s64 seen above. Printed for the record; the per-hit bound is
    asserted where each score is read. Measured on an MI355X when this
    module was written: 1.26e-7 over 2.4M scores, about 80 times inside the
    1e-5 tolerance (one to two f32 ulps)."""
    print(f"\nmax relative GPU score deviation from s64: "
          f"{DEVIATION['max']:.3e} over {DEVIATION['scores']} scores")
    assert DEVIATION["max"] <= ref.REL
