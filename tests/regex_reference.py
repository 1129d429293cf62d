"""Reference for regex queries, independent of csrc/qregex.h: Python's
re.fullmatch over a corpus's term set, then the union of the docs that carry
a matched term.

Python's `re` and the engine's rules agree only on a subset,
and test patterns stay inside it: `\\d \\w \\s` only over ASCII corpora,
`(?i)` only over letters whose lowercase is 1:1, no anchors, no lazy
quantifiers, no back-references.
"""
import re

# Patterns of the device dictionary-scan test (tests/test_regex_gpu.py). The
# scan kernel stages the DFA table in LDS up to 64 KB and reads it from
# global memory above; tests/test_regex_cpu.py asserts, from the compiler's
# own figures, that the first three stay below that and BIG_TABLE above, so
# that both paths keep being exercised.
LDS_TABLE_BYTES = 64 * 1024
BIG_TABLE = ".*\\w[05]\\w{2}"
SMALL_TABLES = ["w.*[05]", "x{40}|a|w000.", "日.|é.*"]


def term_set(docs):
    """docs: one token list per doc -> the sorted distinct terms."""
    return sorted({t for toks in docs for t in toks},
                  key=lambda t: t.encode())


def matched_terms(pattern, terms):
    rx = re.compile(pattern)
    return [t for t in terms if rx.fullmatch(t) is not None]


def regex_hits(docs, pattern):
    """Sorted ids of the docs with at least one term the whole of which
    matches `pattern`."""
    hit = set(matched_terms(pattern, term_set(docs)))
    return [d for d, toks in enumerate(docs) if hit.intersection(toks)]


def assert_selective(docs, pattern):
    """A positive case must select a non-empty proper subset of the terms
    and of the docs — judged by this reference alone."""
    terms = term_set(docs)
    m = matched_terms(pattern, terms)
    assert 0 < len(m) < len(terms), (pattern, len(m), len(terms))
    h = regex_hits(docs, pattern)
    assert 0 < len(h) < len(docs), (pattern, len(h), len(docs))
    return h
