"""Brute-force reference for sloppy phrases and multi-token phrase prefixes
(DESIGN.md §7), over raw token lists. Independent of qast.h and of the
product: positions are token indexes, nothing else is shared.

Slop. For phrase tokens t_0..t_{n-1} and a document, P_i = positions of t_i.
A choice is one p_i in P_i per token, q_i = p_i - i. The document matches
slop S iff some choice has sum_{i>=1} |q_i - q_{i-1}| <= S. Positions need
not be distinct.

Phrase prefix (n >= 2). The last token is a prefix; its expansions are the
first max_expansions terms of the field's dictionary (byte order) that start
with it. A document matches iff t_0..t_{n-2}, e matches consecutively for
some expansion e.
"""
import itertools


def tokens(text):
    """Lowercased alphanumeric runs (the default tokenizer on ASCII)."""
    out, cur = [], []
    for ch in text.lower():
        if ch.isascii() and ch.isalnum():
            cur.append(ch)
        elif cur:
            out.append("".join(cur))
            cur = []
    if cur:
        out.append("".join(cur))
    return out


def _positions(doc_toks, tok):
    return [p for p, t in enumerate(doc_toks) if t == tok]


def min_slop_exhaustive(doc_toks, phrase):
    """Smallest slop at which `doc_toks` matches, trying EVERY choice; None
    when some token is absent. Exponential: small documents only."""
    lists = [_positions(doc_toks, t) for t in phrase]
    if any(not l for l in lists):
        return None
    best = None
    for choice in itertools.product(*lists):
        q = [p - i for i, p in enumerate(choice)]
        cost = sum(abs(q[i] - q[i - 1]) for i in range(1, len(q)))
        best = cost if best is None else min(best, cost)
    return best


def min_slop(doc_toks, phrase):
    """Same value by an integer DP over (token, chosen position)."""
    lists = [_positions(doc_toks, t) for t in phrase]
    if any(not l for l in lists):
        return None
    cost = {p: 0 for p in lists[0]}  # keyed by q = p - i
    for i in range(1, len(phrase)):
        nxt = {}
        for p in lists[i]:
            q = p - i
            nxt[q] = min(c + abs(q - q0) for q0, c in cost.items())
        cost = nxt
    return min(cost.values())


def slop_match(doc_toks, phrase, slop):
    m = min_slop(doc_toks, phrase)
    return m is not None and m <= slop


def slop_hits(docs_toks, phrase, slop):
    return [d for d, t in enumerate(docs_toks) if slop_match(t, phrase, slop)]


def expansions(docs_toks, prefix, max_expansions):
    """First max_expansions dictionary terms, in UTF-8 byte order, that start
    with `prefix`."""
    terms = sorted({t for d in docs_toks for t in d},
                   key=lambda s: s.encode("utf-8"))
    return [t for t in terms if t.startswith(prefix)][:max_expansions]


def prefix_hits(docs_toks, phrase, max_expansions=50):
    assert len(phrase) >= 2
    exps = expansions(docs_toks, phrase[-1], max_expansions)
    out = []
    for d, t in enumerate(docs_toks):
        if any(slop_match(t, phrase[:-1] + [e], 0) for e in exps):
            out.append(d)
    return out
