// Stand-alone driver for csrc/qregex.h (host code that parses untrusted
// patterns), meant to be built with -fsanitize=address,undefined:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all tools/qregex_fuzz_main.cpp -o qregex_fuzz
//   ./qregex_fuzz                 # refusal list + seeded random patterns,
//                                 # on a thread with a 512 KB stack
//   ./qregex_fuzz --table 'RE'    # states / classes / table bytes of one regex
//
// The run feeds the refusal lists of tests/test_regex_cpu.py (long patterns
// of stacked quantifiers and of nested groups included), seeded random
// patterns over the same grammar, and random byte soup through the compiler,
// and every DFA that compiles through the host matcher over all strings of
// [abc] up to length 6 plus a few multi-byte terms. Exit 0 = no crash, every
// refusal refused, and no pattern both compiled and threw.
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../quickwit_amd/csrc/qregex.h"

using qw::rx::Dfa;

static std::vector<std::string> g_terms;

static uint64_t run(const Dfa& d) {
    uint64_t n = 0;
    for (const std::string& t : g_terms)
        n += qw::rx::match(d, (const uint8_t*)t.data(), t.size());
    return n;
}

static std::string random_pattern(std::mt19937& rng, int depth) {
    auto pick = [&](int n) { return int(rng() % uint32_t(n)); };
    static const char* classes[] = {"[ab]", "[^a]", "[b-c]", "[^bc]", "[a-c]",
                                    "\\d", "\\w", "\\S", "[\\x{e9}-\\x{65e5}]"};
    static const char* quants[] = {"", "", "", "*", "+", "?", "{2}", "{1,2}",
                                   "{2,}", "{0,3}"};
    std::string out;
    int pieces = 1 + pick(depth == 0 ? 3 : 2);
    for (int i = 0; i < pieces; ++i) {
        int k = pick(depth < 2 ? 9 : 7);
        if (k < 4) out += char('a' + pick(3));
        else if (k == 4) out += '.';
        else if (k == 5) out += classes[pick(9)];
        else if (k == 6) { out += char('a' + pick(3)); out += char('a' + pick(3)); }
        else {
            out += pick(3) ? "(" : "(?:";
            int alts = 1 + pick(2);
            for (int a = 0; a < alts; ++a) {
                if (a) out += '|';
                out += random_pattern(rng, depth + 1);
            }
            out += ')';
        }
        out += quants[pick(10)];
    }
    return out;
}

static int fuzz();

// the run happens on a thread with a small explicit stack: a pattern that
// recursed deeply would overflow it long before it troubled a main thread
static const size_t FUZZ_STACK_BYTES = 512 * 1024;
static void* fuzz_thread(void* rc) {
    *(int*)rc = fuzz();
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--table") {
        try {
            Dfa d = qw::rx::compile(argv[2]);
            printf("states=%u classes=%u table_bytes=%zu\n", d.n_states,
                   d.n_classes, d.table_bytes());
            return 0;
        } catch (const std::exception& e) {
            printf("refused: %s\n", e.what());
            return 1;
        }
    }
    pthread_attr_t attr;
    pthread_attr_init(&attr);
    pthread_attr_setstacksize(&attr, FUZZ_STACK_BYTES);
    pthread_t th;
    int rc = 1;
    if (pthread_create(&th, &attr, fuzz_thread, &rc) != 0) return 2;
    pthread_join(th, nullptr);
    return rc;
}

static std::string groups_with_stacked_quantifiers(int levels, int per_level) {
    std::string p(size_t(levels), '(');
    p += 'a';
    for (int i = 0; i < levels; ++i) p += ")" + std::string(size_t(per_level), '*');
    return p;
}

static int fuzz() {
    {
        std::vector<std::string> cur{""};
        for (int len = 0; len <= 6; ++len) {
            for (auto& t : cur) g_terms.push_back(t);
            std::vector<std::string> nxt;
            for (auto& t : cur)
                for (char c : {'a', 'b', 'c'}) nxt.push_back(t + c);
            cur.swap(nxt);
        }
        for (const char* t : {"\xc3\xa9", "\xe6\x97\xa5\xe6\x9c\xac",
                              "\xf0\x9f\x98\x80x", "a\xff", "\x80", "12-ab_c"})
            g_terms.push_back(t);
    }
    int bad = 0;
    const char* refusals[] = {
        "red$", "^a", "a\\b", "a*?", "(a)\\1", "(", "[z-a]", "a{3,1}",
        "(a|b)*a(a|b){14}", "a\\B", "a+?", "a??", "a{1,2}?", "(?=a)b",
        "(?<!a)b", "(?-u)a", "a)", "[a", "*a", "a{2000}", "\\pL", "a\\",
        "a\xff", "(?", "(?P<n", "[a-", "[\\", "a{", "a{1", "a{1,", "\\x{",
        "\\x{110000}", "\\ud800", "(?i", "[[:alpha:]]", "[a&&b]", "(((((",
        "(a{1000}){1000}", "\\x4", "(?x)a"};
    // long inputs: nesting by stacked quantifiers or groups, and sheer length
    std::vector<std::string> long_refusals = {
        "a" + std::string(300, '*'), "a" + std::string(15000, '*'),
        "a" + std::string(50000, '*'), "a" + std::string(1000000, '+'),
        std::string(300, '(') + "a" + std::string(300, ')'),
        std::string(15000, '('), std::string(1000000, '('),
        "[" + std::string(20000, 'a') + "]", std::string(20000, '|')};
    // groups and stacked quantifiers mixed: no level is large, the path is
    long_refusals.push_back(groups_with_stacked_quantifiers(100, 150));
    long_refusals.push_back(groups_with_stacked_quantifiers(90, 100));
    long_refusals.push_back(groups_with_stacked_quantifiers(50, 6));
    {
        std::string q(100, '(');
        q += 'a';
        for (int d = 100; d > 0; --d) q += ")" + std::string(size_t(200 - d), '*');
        long_refusals.push_back(q);
        q.clear();
        for (int i = 0; i < 90; ++i) q += "(a|";
        q += 'b';
        for (int i = 0; i < 90; ++i) q += ")+*";
        long_refusals.push_back(q);
    }
    {
        std::string q = "a";
        for (int i = 0; i < 400; ++i) q += "{1}";
        long_refusals.push_back(q);
        q.clear();
        for (int i = 0; i < 400; ++i) q += "(?:";
        long_refusals.push_back(q + "a");
    }
    for (const std::string& p : long_refusals) {
        try {
            Dfa d = qw::rx::compile(p);
            fprintf(stderr, "NOT REFUSED: long pattern of %zu bytes\n", p.size());
            ++bad;
        } catch (const std::exception&) {
        }
    }
    {  // at the nesting limit, not above: compiles and runs
        Dfa d = qw::rx::compile("a" + std::string(150, '*'));
        Dfa g = qw::rx::compile(std::string(90, '(') + "a" + std::string(90, ')'));
        Dfa m = qw::rx::compile(groups_with_stacked_quantifiers(40, 5));
        if (run(d) == 0 || run(g) != 1 || run(m) == 0) ++bad;
    }
    for (const char* p : refusals) {
        try {
            Dfa d = qw::rx::compile(p);
            fprintf(stderr, "NOT REFUSED: %s (%u states)\n", p, d.n_states);
            ++bad;
        } catch (const std::exception&) {
        }
    }
    std::mt19937 rng(20240531);
    uint64_t compiled = 0, refused = 0, hits = 0;
    for (int i = 0; i < 2000; ++i) {
        std::string p = random_pattern(rng, 0);
        try {
            Dfa d = qw::rx::compile(p);
            hits += run(d);
            ++compiled;
        } catch (const std::exception&) {
            ++refused;  // only the state cap can refuse this grammar
        }
    }
    // byte soup from the regex alphabet: mostly malformed, never a crash
    static const char soup[] = "ab.*+?|()[]{}^$\\-,0123:iPs<=!dwx\xc3\xa9\xff";
    for (int i = 0; i < 20000; ++i) {
        std::string p;
        int len = 1 + int(rng() % (i % 10 ? 12 : 200));
        for (int k = 0; k < len; ++k) p += soup[rng() % (sizeof soup - 1)];
        try {
            Dfa d = qw::rx::compile(p);
            hits += run(d);
            ++compiled;
        } catch (const std::exception&) {
            ++refused;
        }
    }
    printf("qregex fuzz: compiled=%llu refused=%llu term_matches=%llu "
           "unrefused_refusals=%d\n",
           (unsigned long long)compiled, (unsigned long long)refused,
           (unsigned long long)hits, bad);
    return bad ? 1 : 0;
}
