"""The four device decoders of 128-posting bitpacked blocks against the
generator's own arrays (tests/posting_reference.py), at every gap width
1..22, every tf width 0..20, every block count on a 32-posting segment edge,
a block spanning hundreds of tiles, and the software pipeline's hand-over
between blocks of different widths:

  decode_term_tile<true>   k_leaf_tile_t, scored term / should count
  decode_term_tile<false>  k_leaf_tile_t, must / must_not bitsets
  union_gap + segment scan k_terms_union_bitmap (regex)
  phrase_doc_at / phrase_tf_prefix            k_phrase_bitmap (slop 0)
  phrase_decode_block / phrase_find_doc       k_phrase_window_bitmap
                                              (slop > 0, phrase prefix)

test_posting_decode_cpu.py has proved the reference and that every corpus
realises the widths it claims; nothing here reads the oracle. Doc ids,
num_hits and hit order are exact and no case is exempt; scores are within
topk_reference.REL of the float64 reference.
"""
import pytest

import posting_reference as ref
from quickwit_amd.api import GpuSearcher, make_leaf_request

pytestmark = pytest.mark.gpu

# largest relative deviation of a GPU score from float64 over the module
DEVIATION = {"max": 0.0, "scores": 0}
SCORE_DESC = [{"field_name": "_score", "sort_order": 1}]


@pytest.fixture(scope="module", autouse=True)
def build_all():
    import __graft_entry__
    __graft_entry__.build()


class Gpu:
    """One device context; each corpus's split is uploaded once."""

    def __init__(self):
        self.searcher = GpuSearcher(device=0)
        self.loaded = set()

    def run(self, corpus, schema, case):
        name, query, kind, expected = case
        if corpus.split_id not in self.loaded:
            self.searcher.add_split(corpus.split_id, corpus.data)
            self.loaded.add(corpus.split_id)
        req = make_leaf_request(
            query, schema, [(corpus.split_id, corpus.num_docs)],
            max_hits=len(expected) + (0 if kind == "scored" else 10),
            sort_fields=SCORE_DESC if kind == "scored" else None)
        try:
            resp = self.searcher.leaf_search(req)
        except RuntimeError as e:
            # a device error is not a mismatch: start nothing more on the GPU
            pytest.exit(f"leaf_search failed, stopping the run: {e}", 3)
        dev = ref.check_response(resp, kind, expected, name)
        if kind == "scored":
            DEVIATION["max"] = max(DEVIATION["max"], dev)
            DEVIATION["scores"] += len(expected)

    def launches(self, kernel):
        try:
            return self.searcher.kernel_stats(kernel)[1]
        except KeyError:  # never launched yet
            return 0


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


CASES_A = ref.cases_a()
CASES_UNION = ref.cases_union()
CASES_B = ref.cases_b()


@pytest.mark.parametrize("case", CASES_A, ids=[c[0] for c in CASES_A])
def test_leaf_tile_decoder(gpu, case):
    """scored-*: decode_term_tile<true>, one term (p0+p1: two), every posting
    returned in reference order. count-*: the same decoder in the should
    count role (minimum_should_match 2 of three). must-* / must_not-*:
    decode_term_tile<false>, each term once in either bitset."""
    gpu.run(ref.corpus_a(), ref.SCHEMA_A, case)


@pytest.mark.parametrize("case", CASES_UNION, ids=[c[0] for c in CASES_UNION])
def test_terms_union_decoder(gpu, case):
    before = gpu.launches("k_terms_union_bitmap")
    gpu.run(ref.corpus_a(), ref.SCHEMA_A, case)
    assert gpu.launches("k_terms_union_bitmap") > before


@pytest.mark.parametrize("case", CASES_B, ids=[c[0] for c in CASES_B])
def test_phrase_decoders(gpu, case):
    exact = case[0].endswith("slop0")  # slop 0: one thread per posting
    kernel = "k_phrase_bitmap" if exact else "k_phrase_window_bitmap"
    before = gpu.launches(kernel)
    gpu.run(ref.corpus_b(), ref.SCHEMA_B, case)
    assert gpu.launches(kernel) > before


def test_zz_score_deviation_report(gpu):
    """Runs last in the module: the largest relative deviation of any GPU
    score from float64 seen above, printed for the record; the per-hit
    bound is asserted where each score is read."""
    print(f"\nmax relative GPU score deviation from float64: "
          f"{DEVIATION['max']:.3e} over {DEVIATION['scores']} scores")
    assert DEVIATION["scores"] > 0 and DEVIATION["max"] <= ref.REL
    assert gpu.launches("k_phrase_bitmap") > 0
    assert gpu.launches("k_phrase_window_bitmap") > 0
