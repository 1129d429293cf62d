"""Regex -> byte DFA compiler (csrc/qregex.h) through its host entry point
qw_regex_match_terms, term for term against Python's re.fullmatch
(tests/regex_reference.py); its refusals; the automatic "(?i)" rule; and the
CPU oracle, which keeps refusing regex queries. No GPU needed."""
import itertools
import random

import pytest

import regex_reference as ref
from quickwit_amd import splitgen
from quickwit_amd.api import (OracleSearcher, make_leaf_request,
                              regex_match_terms, regex_resolve,
                              regex_table_stats)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()


ASCII_TERMS = [
    "", "a", "b", "c", "e", "ef", "eg", "egg", "egxyz", "efg", "event",
    "pushevent", "watchevent", "events", "jour", "journal", "journey", "ajour",
    "ax", "axx", "axxx", "axxxx", "bxx", "cxxx", "dxx", "xx", "abc", "ac",
    "bbbc", "abbccc", "ab", "cab", "rust", "RUST", "Rust-lang", "rustacean",
    "trust", "12-ab", "7-x_y9", "12-", "-ab", "1-2-3", "a b", "tab\there",
    "line\nbreak", "0", "42", "x" * 40, "y" * 200,
]
UTF8_TERMS = [
    "é", "é!", "éa", "日", "日本", "日本語", "😀", "😀x", "x😀", "aé日😀",
    "ß", "ж", "жук", "ǆ", "z", "~", "\x7f", "\u07ff", "\u0800", "\uffff",
    "\U00010000", "a", "ab", "", "\n",
]
PATTERNS_ASCII = [
    ".*event", "event", "jour.*", "e(f|g.*)", "[a-c]x{2,3}", "[^a]+",
    "a?b*c+", "(?i)RUST.*", r"\d+-\w+", r"\s*", r"\S+\s\S+", r"[\d-]+",
    r"\w{2}", "(?:ab|c)+", "x{40}", "y{150,}", ".{0,2}", "(a|b|c)(x+|)",
    r"\D\W?", "[]a]+", "[a\\-c]+", "(?s).*", ".*", "a{2}|b{1,}c",
]
PATTERNS_UTF8 = [
    "日本", "😀", ".", "..", "...", ".*", "(?s).", "[a-日]+", "[é-😀]",
    "[^é]", "[^日]*", "日.?語?", ".😀|😀.", "[\u0080-\u07ff]", "[\u0800-\uffff]+",
    "[\U00010000-\U0010ffff]", "ж.*", "\\x{65e5}", "\\u65E5本", "[^\\x00-\\x7F]+",
]


def check(pattern, terms):
    got = regex_match_terms(pattern, terms)
    exp_terms = set(ref.matched_terms(
        pattern.replace("\\x{65e5}", "\\u65e5"), terms))
    exp = [t in exp_terms for t in terms]
    wrong = [(t, g, e) for t, g, e in zip(terms, got, exp) if g != e]
    assert not wrong, (pattern, wrong[:5])
    return sum(got)


@pytest.mark.parametrize("pattern", PATTERNS_ASCII)
def test_matching_ascii(pattern):
    check(pattern, ASCII_TERMS)


@pytest.mark.parametrize("pattern", PATTERNS_UTF8)
def test_matching_utf8(pattern):
    check(pattern, UTF8_TERMS)


def test_fixed_patterns_are_selective():
    # every fixed pattern tells terms apart (neither all nor none)
    for pats, terms in ((PATTERNS_ASCII, ASCII_TERMS),
                        (PATTERNS_UTF8, UTF8_TERMS)):
        for p in pats:
            if p in ("(?s).*",):
                continue
            n = check(p, terms)
            assert 0 < n < len(terms), (p, n)


# ---------------------------------------------------- random patterns, [abc]
def random_pattern(rng, depth=0):
    def atom():
        k = rng.randrange(9 if depth < 2 else 7)
        if k < 4:
            return rng.choice("abc")
        if k == 4:
            return "."
        if k == 5:
            return rng.choice(["[ab]", "[^a]", "[b-c]", "[^bc]", "[a-c]"])
        if k == 6:
            return rng.choice("abc") + rng.choice("abc")
        alts = [random_pattern(rng, depth + 1)
                for _ in range(rng.randint(1, 2))]
        if rng.random() < 0.2:
            alts.append("")
        return ("(?:" if rng.random() < 0.3 else "(") + "|".join(alts) + ")"

    out = []
    for _ in range(rng.randint(1, 3 if depth == 0 else 2)):
        a = atom()
        q = rng.choice(["", "", "", "*", "+", "?", "{2}", "{1,2}", "{2,}",
                        "{0,3}"])
        out.append(a + q)
    return "".join(out)


ABC_STRINGS = ["".join(s) for n in range(7)
               for s in itertools.product("abc", repeat=n)]


def test_random_patterns_over_abc():
    rng = random.Random(20240531)
    patterns = sorted({random_pattern(rng) for _ in range(330)})
    assert len(patterns) >= 280
    n_some = 0
    for p in patterns:
        n = check(p, ABC_STRINGS)
        n_some += 0 < n < len(ABC_STRINGS)
    assert n_some > len(patterns) // 2  # most patterns tell strings apart


# ------------------------------------------------------------------ refusals
TOO_MANY_STATES = "(a|b)*a(a|b){14}"  # 2^15 subset states
REFUSALS = [
    ("red$", ["$", "assertion"]), ("^a", ["^", "assertion"]),
    ("a\\b", ["\\b", "assertion"]), ("a*?", ["lazy"]),
    ("(a)\\1", ["back-reference"]), ("(", ["unclosed group"]),
    ("[z-a]", ["class range"]), ("a{3,1}", ["repetition range"]),
    (TOO_MANY_STATES, ["too complex"]),
    # further refused constructs of the same families
    ("a\\B", ["assertion"]), ("a+?", ["lazy"]), ("a??", ["lazy"]),
    ("a{1,2}?", ["lazy"]), ("(?=a)b", ["look-around"]),
    ("(?<!a)b", ["look-around"]), ("(?-u)a", ["(?-u)"]), ("a)", [")"]),
    ("[a", ["character class"]), ("*a", ["nothing to repeat"]),
    ("a{2000}", ["too complex"]), ("\\pL", ["\\p"]), ("a\\", ["backslash"]),
]


@pytest.mark.parametrize("pattern,needles", REFUSALS)
def test_refusals_name_the_construct(pattern, needles):
    with pytest.raises(ValueError) as ei:
        regex_match_terms(pattern, ["a", "red", "red$"])
    msg = str(ei.value)
    assert msg.startswith("invalid regex"), msg
    for n in needles:
        assert n in msg, (pattern, msg)


def groups_with_stacked_quantifiers(levels, per_level):
    """`levels` nested groups around "a", each followed by `per_level`
    stacked '*': the AST is levels * per_level REPEAT nodes tall although
    no single group or atom carries many."""
    return "(" * levels + "a" + (")" + "*" * per_level) * levels


LONG_REFUSALS = [
    # stacked quantifiers and groups nest; both are refused long before the
    # nesting could exhaust a stack, whatever the pattern's length
    ("a" + "*" * 300, "nesting too deep"),
    ("a" + "*" * 15000, "nesting too deep"),
    ("a" + "+?" * 10, "lazy"),
    ("a" + "{1}" * 400, "nesting too deep"),
    ("(" * 300 + "a" + ")" * 300, "nesting too deep"),
    # groups and quantifiers mixed: each level stays small, the path is deep
    (groups_with_stacked_quantifiers(100, 150), "nesting too deep"),
    (groups_with_stacked_quantifiers(90, 100), "nesting too deep"),
    (groups_with_stacked_quantifiers(50, 6), "nesting too deep"),
    ("(" * 100 + "a" + "".join(")" + "*" * (200 - d)
                               for d in range(100, 0, -1)), "nesting too deep"),
    # three nodes per level (alternation, two quantifiers): 270 tall
    ("(a|" * 90 + "b" + ")+*" * 90, "nesting too deep"),
    ("(" * 15000, "nesting too deep"),
    ("(?:" * 400 + "a", "nesting too deep"),
    ("a" + "*" * 50000, "too long"),
    ("(" * 100000, "too long"),
    ("[" + "a" * 20000 + "]", "too long"),
    ("a|" * 9000, "too long"),
]


@pytest.mark.parametrize("pattern,needle", LONG_REFUSALS,
                         ids=[str(i) for i in range(len(LONG_REFUSALS))])
def test_long_patterns_are_refused_not_crashing(pattern, needle):
    with pytest.raises(ValueError) as ei:
        regex_match_terms(pattern, ["a"])
    assert needle in str(ei.value), str(ei.value)[:200]


def test_long_but_flat_patterns_compile():
    # nesting and length are what is capped, not size as such
    assert regex_match_terms("a" + "*" * 150, ["", "aaa", "b"]) == \
        [True, True, False]
    deep = "(" * 90 + "a" + ")" * 90
    assert regex_match_terms(deep, ["a", "aa"]) == [True, False]
    mixed = groups_with_stacked_quantifiers(40, 5)  # 200 REPEATs tall
    assert regex_match_terms(mixed, ["", "aaaa", "b"]) == [True, True, False]
    alts = "|".join("w%04d" % i for i in range(2000))  # 12 KB
    assert regex_match_terms(alts, ["w0000", "w1999", "w2000"]) == \
        [True, True, False]


def test_table_sizes_cover_both_scan_paths():
    """The device scan reads the table from LDS up to 64 KB and from global
    memory above. The GPU test's patterns must keep landing on both sides,
    as evaluated on a lowercasing field (automatic "(?i)")."""
    for p in ref.SMALL_TABLES:
        states, classes, nbytes = regex_table_stats(regex_resolve(p, True))
        assert nbytes <= ref.LDS_TABLE_BYTES, (p, states, classes, nbytes)
        assert nbytes >= 256 + 2 * states * classes
    states, classes, nbytes = regex_table_stats(
        regex_resolve(ref.BIG_TABLE, True))
    assert nbytes > ref.LDS_TABLE_BYTES, (states, classes, nbytes)
    assert states <= 10001 and classes <= 256


def test_invalid_utf8_pattern_is_refused():
    with pytest.raises(ValueError):
        regex_match_terms(b"a\xff", ["a"])


# ----------------------------------------------------------- auto-(?i) rule
def test_auto_case_insensitive_rule():
    # RegexQuery::to_resolved: lowercasing (default) vs raw tokenizer
    assert regex_resolve(".*ECONNREFUSED.*", True) == "(?i).*ECONNREFUSED.*"
    assert regex_resolve(".*ECONNREFUSED.*", False) == ".*ECONNREFUSED.*"
    assert regex_resolve("(?i).*ECONNREFUSED.*", True) == "(?i).*ECONNREFUSED.*"
    assert regex_resolve("(?is)abc", True) == "(?is)abc"
    assert regex_resolve("(?mi)abc", True) == "(?mi)abc"
    assert regex_resolve("(?sim)abc", True) == "(?sim)abc"
    # a flag group that is not leading does not count
    assert regex_resolve("abc(?i)def", True) == "(?i)abc(?i)def"
    # other leading flags, or an unclosed "(?", do not count either
    assert regex_resolve("(?s)abc", True) == "(?i)(?s)abc"
    assert regex_resolve("(?", True) == "(?i)(?"
    # and the resolved forms behave: lowercased terms, upper-case pattern
    terms = ["econnrefused", "xeconnrefusedy", "other"]
    assert regex_match_terms(regex_resolve(".*ECONNREFUSED.*", True),
                             terms) == [True, True, False]
    assert regex_match_terms(regex_resolve(".*ECONNREFUSED.*", False),
                             terms) == [False, False, False]
    assert regex_match_terms("abc(?i)def", ["abcDEF", "ABCdef"]) == [True, False]


# -------------------------------------------------------------------- oracle
def test_oracle_keeps_refusing_regex():
    schema = {"timestamp_field": None, "fields": [
        {"name": "f", "type": "text", "tokenizer": "default",
         "record": "position", "fieldnorms": True}]}
    w = splitgen.SplitWriter(schema, "o", store_docs=False)
    w.add_documents([{"f": "x y"}, {"f": "z"}])
    cpu = OracleSearcher()
    cpu.add_split("o", w.finalize())
    for q in ({"type": "regex", "field": "f", "regex": "x"},
              {"type": "user_input", "user_text": "f:/x/",
               "default_fields": ["f"]}):
        try:
            r = cpu.leaf_search(make_leaf_request(q, schema, [("o", 2)]))
            errs = " ".join(f["error"] for f in r.get("failed_splits", []))
            assert r.get("num_hits", 0) == 0, q
        except RuntimeError as e:
            errs = str(e)
        assert "not supported" in errs, (q, errs)
