// Regex -> dense byte DFA for term-dictionary scans (host only, no HIP).
//
// Restates the matching rules of tantivy_fst::Regex as the reference uses it
// (query_ast/regex_query.rs -> AutomatonQuery): the WHOLE term must match,
// the automaton runs over the term's UTF-8 bytes, and everything zero-width
// or non-regular is refused. Pipeline: recursive-descent parser -> Thompson
// NFA over UTF-8 byte ranges -> subset construction -> dense table.
//
//   class_of[256]               byte -> class (bytes no transition tells apart)
//   next[n_states * n_classes]  u16; state 0 = dead, state 1 = start
//   accept[ceil(n_states/64)]   bitset
//
// The same table is walked by rx::match (host) and k_dict_dfa_match (device).
// Limits: DESIGN.md §7.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "qw_unicode.h"

namespace qw {
namespace rx {

constexpr uint32_t MAX_DFA_STATES = 10000;   // "regex too complex" above
constexpr uint32_t MAX_NFA_STATES = 200000;  // bounds {m,n} expansion
constexpr uint32_t MAX_REPEAT = 1000;
constexpr uint32_t MAX_DEPTH = 100;           // nested groups (parser recursion)
// height of the AST along any path, groups, sequences, alternations and
// stacked quantifiers all counted: bounds every recursion over the tree
// (Nfa::build, ~Node)
constexpr uint32_t MAX_HEIGHT = 256;
constexpr size_t MAX_PATTERN_BYTES = 16384;   // "regex too long" above
// subset construction is bounded in work as well as in states: elementary
// steps (NFA states visited by closures, transitions spread over classes)
constexpr uint64_t MAX_DFA_WORK = 400ull * 1000 * 1000;
constexpr uint32_t CP_MAX = 0x10FFFF;

[[noreturn]] inline void fail(const std::string& what) {
    throw std::runtime_error("invalid regex: " + what);
}

// -------------------------------------------------- codepoint range sets
struct Range {
    uint32_t lo, hi;
};
using Class = std::vector<Range>;  // normalised: sorted, disjoint, unmerged gaps

inline void normalise(Class& c) {
    std::sort(c.begin(), c.end(),
              [](const Range& a, const Range& b) { return a.lo < b.lo; });
    Class out;
    for (const Range& r : c) {
        if (!out.empty() && r.lo <= out.back().hi + 1)
            out.back().hi = std::max(out.back().hi, r.hi);
        else out.push_back(r);
    }
    c.swap(out);
}

inline bool contains(const Class& c, uint32_t cp) {
    size_t lo = 0, hi = c.size();
    while (lo < hi) {
        size_t mid = (lo + hi) / 2;
        if (c[mid].hi < cp) lo = mid + 1;
        else hi = mid;
    }
    return lo < c.size() && c[lo].lo <= cp;
}

// complement over the scalar values UTF-8 can carry (surrogates excluded
// when the ranges are encoded)
inline Class negate(Class c) {
    normalise(c);
    Class out;
    uint32_t at = 0;
    for (const Range& r : c) {
        if (r.lo > at) out.push_back({at, r.lo - 1});
        at = r.hi + 1;
    }
    if (at <= CP_MAX) out.push_back({at, CP_MAX});
    return out;
}

// (?i): x joins the class iff lower(x) == lower(y) for some member y, through
// the project's 1:1 lowercase table — the approximation wildcards make too
inline void case_fold(Class& c) {
    normalise(c);
    Class add;
    for (uint32_t i = 0; i < QW_LOWER_N; ++i)
        if (contains(c, QW_LOWER_CP[i])) add.push_back({QW_LOWER_TO[i], QW_LOWER_TO[i]});
    c.insert(c.end(), add.begin(), add.end());
    normalise(c);
    add.clear();
    for (uint32_t i = 0; i < QW_LOWER_N; ++i)
        if (contains(c, QW_LOWER_TO[i])) add.push_back({QW_LOWER_CP[i], QW_LOWER_CP[i]});
    c.insert(c.end(), add.begin(), add.end());
    normalise(c);
}

inline Class class_digit() { return {{'0', '9'}}; }

inline Class class_space() {  // Unicode White_Space
    return {{0x09, 0x0D}, {0x20, 0x20}, {0x85, 0x85}, {0xA0, 0xA0},
            {0x1680, 0x1680}, {0x2000, 0x200A}, {0x2028, 0x2029},
            {0x202F, 0x202F}, {0x205F, 0x205F}, {0x3000, 0x3000}};
}

inline Class class_word() {  // the tokenizer's alnum table plus '_'
    Class c;
    c.push_back({'_', '_'});
    uint32_t start = 0;
    bool in = false;
    for (uint32_t cp = 0; cp <= 0x10000; ++cp) {
        bool a = cp <= 0xFFFF && qw_is_alnum_cp(cp);
        if (a && !in) { start = cp; in = true; }
        if (!a && in) { c.push_back({start, cp - 1}); in = false; }
    }
    normalise(c);
    return c;
}

// ------------------------------------------------------------------- AST
struct Node {
    enum Kind { EMPTY, CLASS, CAT, ALT, REPEAT } kind = EMPTY;
    Class cls;
    std::vector<Node> kids;
    uint32_t min = 0, max = 0;  // REPEAT
    bool unbounded = false;     // REPEAT {m,}
    uint32_t height = 1;        // longest path to a leaf, this node included
};

// height of a node over its kids; refuses a tree taller than MAX_HEIGHT, so
// no tree that leaves the parser can be
inline void set_height(Node& n) {
    uint32_t h = 0;
    for (const Node& k : n.kids) h = std::max(h, k.height);
    n.height = h + 1;
    if (n.height > MAX_HEIGHT) fail("nesting too deep");
}

struct Flags {
    bool ci = false, dotall = false;
};

class Parser {
  public:
    explicit Parser(const std::string& s) : s_(s) {}

    Node parse() {
        if (s_.size() > MAX_PATTERN_BYTES)
            fail("regex too long: more than " +
                 std::to_string(MAX_PATTERN_BYTES) + " bytes");
        Flags fl;
        Node n = alt(fl, 0);
        if (i_ < s_.size()) fail("unopened group: ')' without '('");
        return n;
    }

  private:
    const std::string& s_;
    size_t i_ = 0;

    bool eof() const { return i_ >= s_.size(); }
    char peek() const { return s_[i_]; }

    uint32_t next_cp() {
        unsigned char c = (unsigned char)s_[i_];
        if (c < 0x80) { ++i_; return c; }
        uint32_t cp = 0;
        size_t len = 0;
        if ((c & 0xE0) == 0xC0) { cp = c & 0x1F; len = 2; }
        else if ((c & 0xF0) == 0xE0) { cp = c & 0x0F; len = 3; }
        else if ((c & 0xF8) == 0xF0) { cp = c & 0x07; len = 4; }
        if (!len || i_ + len > s_.size()) fail("pattern is not valid UTF-8");
        for (size_t k = 1; k < len; ++k) {
            unsigned char cc = (unsigned char)s_[i_ + k];
            if ((cc & 0xC0) != 0x80) fail("pattern is not valid UTF-8");
            cp = (cp << 6) | (cc & 0x3F);
        }
        if (cp > CP_MAX || (cp >= 0xD800 && cp <= 0xDFFF))
            fail("pattern is not valid UTF-8");
        i_ += len;
        return cp;
    }

    static Node lit(uint32_t cp, const Flags& fl) {
        Node n;
        n.kind = Node::CLASS;
        n.cls = {{cp, cp}};
        if (fl.ci) case_fold(n.cls);
        return n;
    }

    Node alt(Flags& fl, uint32_t depth) {
        if (depth > MAX_DEPTH) fail("nesting too deep");
        Node a;
        a.kind = Node::ALT;
        a.kids.push_back(cat(fl, depth));
        while (!eof() && peek() == '|') {
            ++i_;
            a.kids.push_back(cat(fl, depth));
        }
        if (a.kids.size() == 1) return std::move(a.kids[0]);
        set_height(a);
        return a;
    }

    Node cat(Flags& fl, uint32_t depth) {
        Node c;
        c.kind = Node::CAT;
        while (!eof() && peek() != '|' && peek() != ')') {
            bool is_flags = false;
            Node atom_n = atom(fl, depth, &is_flags);
            if (is_flags) continue;  // (?i): applies to the rest of the group
            c.kids.push_back(repeat(std::move(atom_n)));
        }
        if (c.kids.empty()) return Node{};
        if (c.kids.size() == 1) return std::move(c.kids[0]);
        set_height(c);
        return c;
    }

    // every quantifier stacked on an atom (a*+?...) nests one REPEAT deeper:
    // set_height counts it on top of whatever the atom already holds
    Node repeat(Node a) {
        while (!eof()) {
            char q = peek();
            uint32_t mn = 0, mx = 0;
            bool unb = false;
            if (q == '*') { ++i_; mn = 0; unb = true; }
            else if (q == '+') { ++i_; mn = 1; unb = true; }
            else if (q == '?') { ++i_; mn = 0; mx = 1; }
            else if (q == '{') {
                size_t save = i_;
                ++i_;
                auto num = [&](uint32_t* out) {
                    if (eof() || !isdigit((unsigned char)peek())) return false;
                    uint64_t v = 0;
                    while (!eof() && isdigit((unsigned char)peek())) {
                        v = v * 10 + uint64_t(s_[i_++] - '0');
                        if (v > MAX_REPEAT)
                            fail("regex too complex: repetition count above " +
                                 std::to_string(MAX_REPEAT));
                    }
                    *out = uint32_t(v);
                    return true;
                };
                if (!num(&mn))
                    fail("repetition '{' at offset " + std::to_string(save) +
                         " needs a count ({m}, {m,} or {m,n})");
                if (!eof() && peek() == ',') {
                    ++i_;
                    if (!num(&mx)) unb = true;
                } else mx = mn;
                if (eof() || peek() != '}') fail("unclosed repetition '{'");
                ++i_;
                if (!unb && mx < mn)
                    fail("invalid repetition range {" + std::to_string(mn) + "," +
                         std::to_string(mx) + "}: max below min");
            } else break;
            if (!eof() && peek() == '?')
                fail("lazy quantifier '" + std::string(1, q) +
                     "?' is not supported");
            Node r;
            r.kind = Node::REPEAT;
            r.min = mn;
            r.max = mx;
            r.unbounded = unb;
            r.kids.push_back(std::move(a));
            set_height(r);
            a = std::move(r);
        }
        return a;
    }

    // leading "?..." of a group, after '(' was consumed. Returns true when
    // the group was a bare flag group "(?flags)" (fully consumed).
    bool group_prefix(Flags& fl, Flags* inner) {
        *inner = fl;
        if (eof() || peek() != '?') return false;
        ++i_;
        if (eof()) fail("unclosed group");
        char c = peek();
        if (c == '=' || c == '!')
            fail("look-around '(?" + std::string(1, c) + "' is not supported");
        if (c == '<' || c == 'P') {
            size_t j = i_ + (c == 'P' ? 1 : 0);
            if (j < s_.size() && s_[j] == '<') {
                if (j + 1 < s_.size() && (s_[j + 1] == '=' || s_[j + 1] == '!'))
                    fail("look-around '(?<" + std::string(1, s_[j + 1]) +
                         "' is not supported");
                size_t close = s_.find('>', j);
                if (close == std::string::npos) fail("unclosed group name");
                i_ = close + 1;  // named group: a plain group here
                return false;
            }
            if (c == 'P') fail("back-reference '(?P=' is not supported");
        }
        if (c == ':') { ++i_; return false; }
        bool neg = false;
        Flags f = fl;
        while (!eof() && peek() != ')' && peek() != ':') {
            char x = s_[i_++];
            if (x == '-') { neg = true; continue; }
            if (x == 'i') f.ci = !neg;
            else if (x == 's') f.dotall = !neg;
            else if (x == 'm') { /* multi-line: no anchors exist to change */ }
            else if (x == 'u') {
                if (neg) fail("byte classes '(?-u)' are not supported");
            } else
                fail("flag '" + std::string(1, x) + "' is not supported");
        }
        if (eof()) fail("unclosed group");
        if (peek() == ')') {
            ++i_;
            fl = f;
            return true;
        }
        ++i_;  // ':'
        *inner = f;
        return false;
    }

    Node atom(Flags& fl, uint32_t depth, bool* is_flags) {
        char c = peek();
        if (c == '(') {
            ++i_;
            Flags inner;
            if (group_prefix(fl, &inner)) {
                *is_flags = true;
                return Node{};
            }
            Node n = alt(inner, depth + 1);
            if (eof() || peek() != ')') fail("unclosed group: '(' without ')'");
            ++i_;
            return n;
        }
        if (c == '[') return bracket(fl);
        if (c == '.') {
            ++i_;
            Node n;
            n.kind = Node::CLASS;
            if (fl.dotall) n.cls = {{0, CP_MAX}};
            else n.cls = {{0, '\n' - 1}, {'\n' + 1, CP_MAX}};
            return n;
        }
        if (c == '^' || c == '$')
            fail("zero-width assertion '" + std::string(1, c) +
                 "' is not supported (the whole term always has to match)");
        if (c == '*' || c == '+' || c == '?')
            fail("repetition operator '" + std::string(1, c) +
                 "' has nothing to repeat");
        if (c == '{') fail("repetition '{' has nothing to repeat");
        if (c == '\\') {
            Node n;
            n.kind = Node::CLASS;
            uint32_t cp = 0;
            if (escape(fl, &n.cls, &cp, false)) return n;
            return lit(cp, fl);
        }
        return lit(next_cp(), fl);
    }

    static int hexval(char c) {
        if (c >= '0' && c <= '9') return c - '0';
        if (c >= 'a' && c <= 'f') return c - 'a' + 10;
        if (c >= 'A' && c <= 'F') return c - 'A' + 10;
        return -1;
    }

    uint32_t hex_escape(char kind) {
        uint32_t v = 0;
        if (!eof() && peek() == '{') {
            ++i_;
            size_t n = 0;
            while (!eof() && peek() != '}') {
                int h = hexval(s_[i_++]);
                if (h < 0 || ++n > 6) fail("invalid hex escape");
                v = v * 16 + uint32_t(h);
            }
            if (eof() || !n) fail("invalid hex escape");
            ++i_;
        } else {
            size_t want = kind == 'x' ? 2 : kind == 'u' ? 4 : 8;
            for (size_t k = 0; k < want; ++k) {
                if (eof()) fail("invalid hex escape");
                int h = hexval(s_[i_++]);
                if (h < 0) fail("invalid hex escape");
                v = v * 16 + uint32_t(h);
            }
        }
        if (v > CP_MAX || (v >= 0xD800 && v <= 0xDFFF))
            fail("hex escape is not a Unicode scalar value");
        return v;
    }

    // after '\\' at i_. Returns true and fills *cls for a class escape,
    // false and *cp for a single codepoint.
    bool escape(const Flags& fl, Class* cls, uint32_t* cp, bool in_class) {
        ++i_;
        if (eof()) fail("trailing backslash");
        char e = peek();
        if (e >= '1' && e <= '9')
            fail("back-reference '\\" + std::string(1, e) + "' is not supported");
        if (e == 'b' || e == 'B' || e == 'A' || e == 'z' || e == 'Z' || e == 'G') {
            if (!(in_class && e == 'b'))
                fail("zero-width assertion '\\" + std::string(1, e) +
                     "' is not supported");
        }
        if (e == 'k') fail("back-reference '\\k' is not supported");
        if (e == 'p' || e == 'P')
            fail("Unicode property class '\\" + std::string(1, e) +
                 "' is not supported");
        bool neg = false;
        switch (e) {
            case 'D': neg = true; [[fallthrough]];
            case 'd': ++i_; *cls = class_digit(); break;
            case 'W': neg = true; [[fallthrough]];
            case 'w': ++i_; *cls = class_word(); break;
            case 'S': neg = true; [[fallthrough]];
            case 's': ++i_; *cls = class_space(); break;
            case 'n': ++i_; *cp = '\n'; return false;
            case 't': ++i_; *cp = '\t'; return false;
            case 'r': ++i_; *cp = '\r'; return false;
            case 'f': ++i_; *cp = '\f'; return false;
            case 'v': ++i_; *cp = '\v'; return false;
            case 'a': ++i_; *cp = 0x07; return false;
            case '0': ++i_; *cp = 0; return false;
            case 'x': case 'u': case 'U':
                ++i_;
                *cp = hex_escape(e);
                return false;
            default:
                if (isalnum((unsigned char)e))
                    fail("escape '\\" + std::string(1, e) + "' is not supported");
                *cp = next_cp();  // escaped punctuation (or non-ASCII): literal
                return false;
        }
        if (fl.ci) case_fold(*cls);
        if (neg) *cls = negate(*cls);
        return true;
    }

    Node bracket(const Flags& fl) {
        ++i_;  // '['
        bool neg = false;
        if (!eof() && peek() == '^') { neg = true; ++i_; }
        Class c;
        bool first = true;
        for (;;) {
            if (eof()) fail("unclosed character class: '[' without ']'");
            char ch = peek();
            if (ch == ']' && !first) { ++i_; break; }
            first = false;
            if (ch == '[') {
                if (i_ + 1 < s_.size() && s_[i_ + 1] == ':')
                    fail("POSIX class '[:name:]' is not supported");
                fail("nested character class is not supported");
            }
            if (ch == '&' && i_ + 1 < s_.size() && s_[i_ + 1] == '&')
                fail("class intersection '&&' is not supported");
            uint32_t lo = 0;
            if (ch == '\\') {
                Class sub;
                if (escape(Flags{}, &sub, &lo, true)) {
                    c.insert(c.end(), sub.begin(), sub.end());
                    continue;
                }
            } else lo = next_cp();
            uint32_t hi = lo;
            if (i_ + 1 < s_.size() && peek() == '-' && s_[i_ + 1] != ']') {
                ++i_;
                if (peek() == '\\') {
                    Class sub;
                    if (escape(Flags{}, &sub, &hi, true))
                        fail("invalid class range: a class cannot end a range");
                } else if (peek() == '[') {
                    fail("nested character class is not supported");
                } else hi = next_cp();
                if (hi < lo) {
                    std::string a, b;
                    qw_utf8_put(a, lo);
                    qw_utf8_put(b, hi);
                    fail("invalid class range '" + a + "-" + b +
                         "': start above end");
                }
            }
            c.push_back({lo, hi});
        }
        normalise(c);
        if (fl.ci) case_fold(c);
        if (neg) c = negate(c);
        Node n;
        n.kind = Node::CLASS;
        n.cls = std::move(c);
        return n;
    }

    static void qw_utf8_put(std::string& out, uint32_t cp) {
        if (cp < 0x80) out.push_back(char(cp));
        else if (cp < 0x800) {
            out.push_back(char(0xC0 | (cp >> 6)));
            out.push_back(char(0x80 | (cp & 0x3F)));
        } else if (cp < 0x10000) {
            out.push_back(char(0xE0 | (cp >> 12)));
            out.push_back(char(0x80 | ((cp >> 6) & 0x3F)));
            out.push_back(char(0x80 | (cp & 0x3F)));
        } else {
            out.push_back(char(0xF0 | (cp >> 18)));
            out.push_back(char(0x80 | ((cp >> 12) & 0x3F)));
            out.push_back(char(0x80 | ((cp >> 6) & 0x3F)));
            out.push_back(char(0x80 | (cp & 0x3F)));
        }
    }
};

// ------------------------------------------------ UTF-8 range sequences
struct ByteSeq {
    uint8_t n;
    uint8_t lo[4], hi[4];
};

inline size_t utf8_enc(uint32_t cp, uint8_t* b) {
    if (cp < 0x80) { b[0] = uint8_t(cp); return 1; }
    if (cp < 0x800) {
        b[0] = uint8_t(0xC0 | (cp >> 6));
        b[1] = uint8_t(0x80 | (cp & 0x3F));
        return 2;
    }
    if (cp < 0x10000) {
        b[0] = uint8_t(0xE0 | (cp >> 12));
        b[1] = uint8_t(0x80 | ((cp >> 6) & 0x3F));
        b[2] = uint8_t(0x80 | (cp & 0x3F));
        return 3;
    }
    b[0] = uint8_t(0xF0 | (cp >> 18));
    b[1] = uint8_t(0x80 | ((cp >> 12) & 0x3F));
    b[2] = uint8_t(0x80 | ((cp >> 6) & 0x3F));
    b[3] = uint8_t(0x80 | (cp & 0x3F));
    return 4;
}

// [lo, hi] of one encoded length -> sequences of per-byte ranges whose
// product is exactly the range (split where a continuation byte would
// otherwise have to depend on the byte before it)
inline void utf8_split(uint32_t lo, uint32_t hi, size_t n, std::vector<ByteSeq>& out) {
    for (size_t i = 1; i < n; ++i) {
        uint32_t m = (1u << (6 * i)) - 1u;
        if ((lo & ~m) != (hi & ~m)) {
            if ((lo & m) != 0) {
                utf8_split(lo, lo | m, n, out);
                utf8_split((lo | m) + 1, hi, n, out);
                return;
            }
            if ((hi & m) != m) {
                utf8_split(lo, (hi & ~m) - 1, n, out);
                utf8_split(hi & ~m, hi, n, out);
                return;
            }
        }
    }
    ByteSeq s{};
    s.n = uint8_t(n);
    utf8_enc(lo, s.lo);
    utf8_enc(hi, s.hi);
    out.push_back(s);
}

inline void utf8_sequences(const Class& c, std::vector<ByteSeq>& out) {
    static const uint32_t edge_lo[4] = {0, 0x80, 0x800, 0x10000};
    static const uint32_t edge_hi[4] = {0x7F, 0x7FF, 0xFFFF, CP_MAX};
    for (const Range& r : c)
        for (size_t n = 0; n < 4; ++n) {
            uint32_t lo = std::max(r.lo, edge_lo[n]), hi = std::min(r.hi, edge_hi[n]);
            if (lo > hi) continue;
            if (n == 2) {  // cut the surrogates out
                if (lo < 0xD800)
                    utf8_split(lo, std::min<uint32_t>(hi, 0xD7FF), 3, out);
                if (hi > 0xDFFF)
                    utf8_split(std::max<uint32_t>(lo, 0xE000), hi, 3, out);
            } else utf8_split(lo, hi, n + 1, out);
        }
}

// ------------------------------------------------------------------- NFA
struct NState {
    std::vector<uint32_t> eps;
    bool has_byte = false;
    uint8_t lo = 0, hi = 0;
    uint32_t to = 0;
};

struct Nfa {
    std::vector<NState> st;
    uint32_t add() {
        if (st.size() >= MAX_NFA_STATES)
            fail("regex too complex: more than " + std::to_string(MAX_NFA_STATES) +
                 " NFA states");
        st.emplace_back();
        return uint32_t(st.size() - 1);
    }
    // compile `n` between fresh states; returns {start, end}
    std::pair<uint32_t, uint32_t> build(const Node& n) {
        uint32_t s = add(), e = add();
        switch (n.kind) {
            case Node::EMPTY:
                st[s].eps.push_back(e);
                break;
            case Node::CLASS: {
                std::vector<ByteSeq> seqs;
                utf8_sequences(n.cls, seqs);
                // sequences with the same tail of byte ranges share the
                // states of that tail (most multi-byte sequences end in
                // [80-BF]): built back to front, keyed by the tail
                std::map<std::vector<uint8_t>, uint32_t> tails;
                for (const ByteSeq& q : seqs) {
                    uint32_t nx = e;
                    std::vector<uint8_t> key;
                    for (int k = int(q.n) - 1; k >= 0; --k) {
                        key.push_back(q.lo[k]);
                        key.push_back(q.hi[k]);
                        auto it = tails.find(key);
                        if (it == tails.end()) {
                            uint32_t cur = add();
                            st[cur].has_byte = true;
                            st[cur].lo = q.lo[k];
                            st[cur].hi = q.hi[k];
                            st[cur].to = nx;
                            it = tails.emplace(key, cur).first;
                            if (k == 0) st[s].eps.push_back(cur);
                        }
                        nx = it->second;
                    }
                }
                break;
            }
            case Node::CAT: {
                uint32_t cur = s;
                for (const Node& k : n.kids) {
                    auto f = build(k);
                    st[cur].eps.push_back(f.first);
                    cur = f.second;
                }
                st[cur].eps.push_back(e);
                break;
            }
            case Node::ALT:
                for (const Node& k : n.kids) {
                    auto f = build(k);
                    st[s].eps.push_back(f.first);
                    st[f.second].eps.push_back(e);
                }
                break;
            case Node::REPEAT: {
                const Node& k = n.kids[0];
                uint32_t cur = s;
                for (uint32_t i = 0; i < n.min; ++i) {
                    auto f = build(k);
                    st[cur].eps.push_back(f.first);
                    cur = f.second;
                }
                if (n.unbounded) {
                    auto f = build(k);
                    st[cur].eps.push_back(f.first);
                    st[cur].eps.push_back(e);
                    st[f.second].eps.push_back(f.first);
                    st[f.second].eps.push_back(e);
                } else {
                    for (uint32_t i = n.min; i < n.max; ++i) {
                        auto f = build(k);
                        st[cur].eps.push_back(f.first);
                        st[cur].eps.push_back(e);
                        cur = f.second;
                    }
                    st[cur].eps.push_back(e);
                }
                break;
            }
        }
        return {s, e};
    }
};

// ------------------------------------------------------------------- DFA
struct Dfa {
    uint8_t class_of[256];
    uint32_t n_classes = 0;
    uint32_t n_states = 0;          // including dead state 0
    std::vector<uint16_t> next;     // [n_states * n_classes]
    std::vector<uint64_t> accept;   // bit s = state s accepts

    bool accepts(uint32_t s) const { return (accept[s >> 6] >> (s & 63)) & 1u; }
    // size of the table image the device reads: class_of | next | pad to 8
    // | accept words (product.cpp dfa_table_image)
    size_t accept_off() const { return (256 + next.size() * 2 + 7) / 8 * 8; }
    size_t table_bytes() const { return accept_off() + accept.size() * 8; }
};

inline Dfa compile(const std::string& pattern) {
    Node ast = Parser(pattern).parse();
    Nfa nfa;
    auto frag = nfa.build(ast);
    const uint32_t match_state = frag.second;
    const size_t N = nfa.st.size();

    Dfa d;
    // byte classes: a class boundary wherever some transition starts or ends
    bool cut[257] = {false};
    for (const NState& s : nfa.st)
        if (s.has_byte) {
            cut[s.lo] = true;
            cut[uint32_t(s.hi) + 1] = true;
        }
    uint32_t nc = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        if (b == 0 || cut[b]) ++nc;
        d.class_of[b] = uint8_t(nc - 1);
    }
    d.n_classes = nc;

    // a DFA state is the sorted set of NFA states that can act: those with
    // a byte transition, and the match state
    std::vector<uint32_t> stack, mark(N, 0);
    uint32_t epoch = 0;
    uint64_t work = 0;
    auto spend = [&](uint64_t n) {
        work += n;
        if (work > MAX_DFA_WORK)
            fail("regex too complex: DFA construction work bound exceeded");
    };
    auto closure = [&](const std::vector<uint32_t>& seeds) {
        ++epoch;
        spend(seeds.size());
        std::vector<uint32_t> out;
        stack.assign(seeds.begin(), seeds.end());
        while (!stack.empty()) {
            uint32_t s = stack.back();
            stack.pop_back();
            if (mark[s] == epoch) continue;
            mark[s] = epoch;
            spend(1);
            if (nfa.st[s].has_byte || s == match_state) out.push_back(s);
            for (uint32_t t : nfa.st[s].eps)
                if (mark[t] != epoch) stack.push_back(t);
        }
        std::sort(out.begin(), out.end());
        return out;
    };
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> sets;
    sets.emplace_back();  // state 0: dead
    ids.emplace(sets[0], 0u);
    auto intern = [&](std::vector<uint32_t> set) -> uint32_t {
        spend(set.size());
        auto it = ids.find(set);
        if (it != ids.end()) return it->second;
        if (sets.size() > MAX_DFA_STATES)
            fail("regex too complex: more than " + std::to_string(MAX_DFA_STATES) +
                 " DFA states");
        uint32_t id = uint32_t(sets.size());
        ids.emplace(set, id);
        sets.push_back(std::move(set));
        return id;
    };
    {
        std::vector<uint32_t> start = closure({frag.first});
        if (start.empty()) {  // cannot happen (the match state is reachable
                              // or a byte is needed), but keep state 1 = start
            sets.emplace_back();
        } else intern(std::move(start));
    }
    // each member's transition covers whole classes (class cuts sit on
    // every range end), so spread its target over [class(lo), class(hi)]
    // once per member instead of testing every member for every class
    std::vector<std::vector<uint32_t>> seeds(nc);
    for (uint32_t cur = 1; cur < sets.size(); ++cur) {
        d.next.resize(size_t(cur + 1) * nc, 0);
        for (auto& v : seeds) v.clear();
        const std::vector<uint32_t> members = sets[cur];  // sets may grow
        for (uint32_t s : members) {
            const NState& ns = nfa.st[s];
            if (!ns.has_byte) continue;
            uint32_t c0 = d.class_of[ns.lo], c1 = d.class_of[ns.hi];
            spend(c1 - c0 + 1);
            for (uint32_t c = c0; c <= c1; ++c) seeds[c].push_back(ns.to);
        }
        // many classes of one state lead to the same targets: close each
        // distinct seed list once
        std::map<std::vector<uint32_t>, uint32_t> seen;
        for (uint32_t c = 0; c < nc; ++c) {
            uint32_t to = 0;
            if (!seeds[c].empty()) {
                spend(seeds[c].size());
                auto it = seen.find(seeds[c]);
                if (it == seen.end())
                    it = seen.emplace(seeds[c], intern(closure(seeds[c]))).first;
                to = it->second;
            }
            d.next[size_t(cur) * nc + c] = uint16_t(to);
        }
    }
    d.n_states = uint32_t(sets.size());
    d.next.resize(size_t(d.n_states) * nc, 0);
    d.accept.assign((d.n_states + 63) / 64, 0);
    for (uint32_t s = 1; s < d.n_states; ++s)
        if (std::binary_search(sets[s].begin(), sets[s].end(), match_state))
            d.accept[s >> 6] |= 1ull << (s & 63);
    return d;
}

// compile() memoised per process, refusals included: a query's regex is
// compiled when it is planned and again for every split and segment it is
// evaluated on. Entries are dropped wholesale once they hold 32 MB.
inline std::shared_ptr<const Dfa> compile_cached(const std::string& pattern) {
    struct Entry {
        std::shared_ptr<const Dfa> dfa;
        std::string error;
    };
    static std::mutex mu;
    static std::map<std::string, Entry> cache;
    static size_t bytes = 0;
    // never a key of the cache: an over-long pattern is refused up front
    if (pattern.size() > MAX_PATTERN_BYTES)
        return std::make_shared<const Dfa>(compile(pattern));  // throws
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find(pattern);
        if (it != cache.end()) {
            if (!it->second.dfa) throw std::runtime_error(it->second.error);
            return it->second.dfa;
        }
    }
    Entry e;
    try {
        e.dfa = std::make_shared<const Dfa>(compile(pattern));
    } catch (const std::exception& ex) {
        e.error = ex.what();
    }
    {
        std::lock_guard<std::mutex> g(mu);
        size_t sz = pattern.size() + e.error.size() +
                    (e.dfa ? e.dfa->table_bytes() : 0) + 64;
        if (bytes + sz > (32u << 20)) {
            cache.clear();
            bytes = 0;
        }
        if (cache.emplace(pattern, e).second) bytes += sz;
    }
    if (!e.dfa) throw std::runtime_error(e.error);
    return e.dfa;
}

inline bool match(const Dfa& d, const uint8_t* s, size_t n) {
    uint32_t st = 1;
    for (size_t i = 0; i < n && st; ++i)
        st = d.next[size_t(st) * d.n_classes + d.class_of[s[i]]];
    return d.accepts(st);
}

// does a leading "(?flags)" group already carry `i`? (regex_query.rs
// regex_has_case_insensitive_flag: the text up to the first ')' after "(?")
inline bool has_case_insensitive_flag(const std::string& re) {
    if (re.compare(0, 2, "(?") != 0) return false;
    size_t end = re.find(')', 2);
    if (end == std::string::npos) return false;
    return re.find('i', 2) < end;
}

// RegexQuery::to_resolved: a lowercasing tokenizer makes the regex
// case-insensitive unless it already says so
inline std::string resolve(const std::string& re, bool tokenizer_lowercases) {
    if (tokenizer_lowercases && !has_case_insensitive_flag(re)) return "(?i)" + re;
    return re;
}

}  // namespace rx
}  // namespace qw
