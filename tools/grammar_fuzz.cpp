// A stand-alone driver for the grammar compiler (kjarni_amd/csrc/grammar.cpp), meant to be built with the sanitizers and run on
// the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikjarni_amd/csrc \
//       tools/grammar_fuzz.cpp kjarni_amd/csrc/grammar.cpp -o /tmp/grammar_fuzz && /tmp/grammar_fuzz 4000
//
// It feeds the compiler generated grammars (random rule lists whose patterns are random trees over the pattern syntax with rule
// calls mixed in), mutations of them and of a seed list (bytes deleted, duplicated, replaced by metacharacters or by arbitrary
// bytes; rules dropped, doubled and renamed), and random byte strings as patterns.  Every grammar either compiles -- then the
// table is checked for shape (every entry names states of the table, the flags say what the entries say) and random strings are
// walked through it, as plain strings and as single tokens -- or ends in a GrammarError; anything else (another exception, a
// sanitizer report, a crash) fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <utility>
#include <vector>

#include "grammar.h"

namespace {

using Rules = std::vector<std::pair<std::string, std::string>>;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next()
    {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 16);
    }
    uint32_t below(uint32_t n) { return n ? next() % n : 0; }
    bool coin(uint32_t one_in) { return below(one_in) == 0; }
};

const char* const kAtoms[] = {"a", "b", "0", " ", "\\d", "\\w", ".", "\\{", "\\}", "\\[", "\\]", "\\(", "\\)", ",", ":", "\"", "[a-z]", "[^\"\\\\]", "\xC3\xA9", "\xF0\x9F\x98\x80"};
const char* const kQuants[] = {"*", "+", "?", "{0}", "{2}", "{0,2}", "{2,5}", "{40}"};
const char* const kNames[] = {"a", "b", "c", "value", "_x1", "R"};
const char kMeta[] = "\\.^$*+?{}[]()|-,&";

const Rules kSeeds[] = {
    {{"s", "(?:\\((?&s)\\)|\\[(?&s)\\])*"}},
    {{"s", "a(?&s)b|ab"}},
    {{"s", "a(?&s)?b"}},
    {{"v", "[0-9]+|\\[(?:(?&v)(?:,(?&v))*)?\\]"}},
    {{"a", "x(?&b)"}, {"b", "(?&c)y"}, {"c", "(?&d)"}, {"d", "z+"}},
    {{"value", "(?&object)|(?&array)|\"[a-z]*\"|-?[0-9]+|true|false|null"}, {"object", "\\{(?:\"[a-z]*\":(?&value)(?:,\"[a-z]*\":(?&value))*)?\\}"},
     {"array", "\\[(?:(?&value)(?:,(?&value))*)?\\]"}},
    {{"s", "(?&s)a|a"}},
    {{"s", "(?&t)"}, {"t", "(?&s)x|y"}},
    {{"s", "a(?&t)"}, {"t", "b*"}},
    {{"s", "a(?&t)b"}, {"t", "b+"}},
    {{"s", "a|(?&t)"}, {"t", "ab"}},
    {{"s", "(?&t)|(?&u)"}, {"t", "ab"}, {"u", "ac"}},
    {{"s", "a(?&s)"}},
    {{"s", "a(?&nope)"}},
    {{"s", "a"}, {"s", "b"}},
    {{"9s", "a"}},
    {{"s", "(?&"}},
    {{"s", "(?&)"}},
    {{"s", "(?&a b)"}},
    {{"s", "[ab]*a[ab]{12}"}},
    {{"s", "x"}, {"unused", "(?&unused)"}},
};

std::string tree(Rng& r, int depth, int n_rules)
{
    const uint32_t pick = r.below(depth <= 0 ? 3 : 9);
    std::string s;
    if (pick < 2) {
        s = kAtoms[r.below(sizeof(kAtoms) / sizeof(kAtoms[0]))];
    } else if (pick == 2) {
        s = std::string("(?&") + kNames[r.below((uint32_t)n_rules + (r.coin(12) ? 1 : 0)) % (sizeof(kNames) / sizeof(kNames[0]))] + ")";
    } else if (pick < 5) {
        const int n = 1 + (int)r.below(4);
        for (int i = 0; i < n; ++i) s += tree(r, depth - 1, n_rules);
    } else if (pick < 7) {
        const int n = 2 + (int)r.below(3);
        s = "(?:";
        for (int i = 0; i < n; ++i) s += (i ? "|" : "") + tree(r, depth - 1, n_rules);
        s += ")";
    } else {
        s = "(?:" + tree(r, depth - 1, n_rules) + ")";
    }
    if (r.coin(4)) s += kQuants[r.below(sizeof(kQuants) / sizeof(kQuants[0]))];
    return s;
}

Rules generate(Rng& r)
{
    const int n = 1 + (int)r.below(5);
    Rules g;
    for (int i = 0; i < n; ++i) g.emplace_back(kNames[i], tree(r, 1 + (int)r.below(3), n));
    return g;
}

// Grammars that are likely to compile: every call sits behind its own opening byte.
Rules generate_guarded(Rng& r)
{
    const int n = 1 + (int)r.below(4);
    const char* const open[] = {"\\(", "\\[", "\\{", "<"};
    const char* const close[] = {"\\)", "\\]", "\\}", ">"};
    Rules g;
    for (int i = 0; i < n; ++i) {
        std::string p = "(?:[a-z0-9]";
        for (int k = 0; k < n; ++k)
            if (r.coin(2) || k == i) p += std::string("|") + open[k] + "(?:(?&" + kNames[k] + ")(?:,(?&" + kNames[k] + "))*)?" + close[k];
        p += ")";
        g.emplace_back(kNames[i], p);
    }
    return g;
}

void mutate(Rng& r, Rules& g)
{
    const int edits = 1 + (int)r.below(4);
    for (int e = 0; e < edits; ++e) {
        if (g.empty()) return;
        const size_t which = r.below((uint32_t)g.size());
        std::string& s = r.coin(8) ? g[which].first : g[which].second;
        const size_t at = s.empty() ? 0 : r.below((uint32_t)s.size());
        switch (r.below(8)) {
        case 0:
            if (!s.empty()) s.erase(at, 1 + r.below(3));
            break;
        case 1:
            if (!s.empty()) s.insert(at, s.substr(at, 1 + r.below(6)));
            break;
        case 2: s.insert(at, 1, kMeta[r.below(sizeof(kMeta) - 1)]); break;
        case 3: s.insert(at, 1, (char)r.below(256)); break;
        case 4: s.insert(at, std::string("(?&") + kNames[r.below(sizeof(kNames) / sizeof(kNames[0]))] + ")"); break;
        case 5: g.erase(g.begin() + (long)which); break;
        case 6: g.push_back(g[which]); break;
        default:
            if (!s.empty()) s[at] = kMeta[r.below(sizeof(kMeta) - 1)];
            break;
        }
    }
}

struct Tally {
    size_t compiled = 0, refused = 0, max_states = 0, walked = 0, survived = 0, deepest = 0;
};

void complain(const char* what, const Rules& g)
{
    std::fprintf(stderr, "%s for the grammar:\n", what);
    for (const auto& rule : g) std::fprintf(stderr, "  %s := %s\n", rule.first.c_str(), rule.second.c_str());
}

bool run_one(const Rules& g, Rng& r, Tally& tally)
{
    try {
        const kjarni::Grammar m = kjarni::compile_grammar(g);
        const size_t S = (size_t)m.states();
        bool ok = S >= 1 && S <= (size_t)kjarni::kGrammarMaxStates && m.action.size() == S * 256 && m.rule_of.size() == S && !m.rules.empty() &&
                  m.rules.size() <= g.size() && m.rule_of[0] == 0;
        bool any_accepting = false;
        for (size_t q = 0; ok && q < S; ++q) {
            bool any = false;
            ok = ok && m.rule_of[q] < m.rules.size();
            for (int b = 0; ok && b < 256; ++b) {
                const uint32_t a = m.action[q * 256 + (size_t)b];
                const uint32_t kind = a >> 30, next = a & 0xFFFu, ret = (a >> 12) & 0xFFFu;
                if (kind == 0) {
                    ok = a == 0;
                } else if (kind == 1) {
                    ok = next < S && (a & 0x3FFFF000u) == 0 && m.rule_of[next] == m.rule_of[q];
                    any = true;
                } else if (kind == 2) {
                    // the callee's start state is the first state of its rule; the return state is one of the caller's
                    ok = next < S && ret < S && (a & 0x3F000000u) == 0 && m.rule_of[ret] == m.rule_of[q] && (next == 0 || m.rule_of[next - 1] != m.rule_of[next]);
                    any = true;
                } else {
                    ok = false;
                }
            }
            any_accepting = any_accepting || (m.flags[q] & kjarni::kGrammarAccepting);
            ok = ok && ((m.flags[q] & kjarni::kGrammarNoOut) != 0) == !any && (m.flags[q] & ~3u) == 0;
        }
        ok = ok && any_accepting;
        if (!ok) {
            complain("malformed table", g);
            return false;
        }
        // walks, with bytes of the patterns themselves so that some of them survive; each string as a plain string, then again as
        // one token from wherever the first walk ended
        std::string pool;
        for (const auto& rule : g) pool += rule.second;
        for (int k = 0; k < 8; ++k) {
            uint8_t buf[96];
            const size_t n = r.below(sizeof(buf));
            for (size_t i = 0; i < n; ++i) buf[i] = pool.empty() || r.coin(5) ? (uint8_t)r.below(256) : (uint8_t)pool[r.below((uint32_t)pool.size())];
            kjarni::GrammarConfig c;
            ++tally.walked;
            size_t done = 0;
            while (done < n) {  // byte by byte, to keep the longest live prefix
                kjarni::GrammarConfig next = c;
                if (!m.walk(&next, buf + done, 1, false)) break;
                c = next;
                ++done;
                if (!m.valid(c)) {
                    complain("a walk left the table", g);
                    return false;
                }
            }
            if (done == n) ++tally.survived;
            if ((size_t)c.depth > tally.deepest) tally.deepest = (size_t)c.depth;
            (void)m.accepted(c);
            (void)m.closed(c);
            kjarni::GrammarConfig t = c;
            if (m.walk(&t, buf, n, true) && !m.valid(t)) {
                complain("a token walk left the table", g);
                return false;
            }
        }
        kjarni::GrammarConfig bad;
        bad.state = (uint32_t)S;
        const uint8_t z = 0;
        if (m.walk(&bad, &z, 1, false)) {
            complain("a walk from no state succeeded", g);
            return false;
        }
        ++tally.compiled;
        if (S > tally.max_states) tally.max_states = S;
    } catch (const kjarni::GrammarError&) {
        ++tally.refused;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception '%s'\n", e.what());
        complain("unexpected exception", g);
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    const size_t rounds = argc > 1 ? (size_t)std::strtoull(argv[1], nullptr, 10) : 4000;
    Rng r(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    Tally tally;
    size_t n = 0;
    for (const Rules& seed : kSeeds) {
        ++n;
        if (!run_one(seed, r, tally)) return 1;
    }
    {  // the limits: no rule, too many rules, a long chain of calls, deep nesting in one pattern, a long name
        Rules many, chain;
        for (int i = 0; i < 300; ++i) many.emplace_back("r" + std::to_string(i), "a");
        for (int i = 0; i < 256; ++i) chain.emplace_back("r" + std::to_string(i), i == 255 ? std::string("a") : "(?&r" + std::to_string(i + 1) + ")");
        for (const Rules& g : {Rules{}, many, chain, Rules{{"s", std::string(3000, '(') + "(?&s)" + std::string(3000, ')')}}, Rules{{std::string(5000, 'n'), "a"}},
                               Rules{{"s", "(?&" + std::string(5000, 'n') + ")"}}}) {
            ++n;
            if (!run_one(g, r, tally)) return 1;
        }
    }
    for (size_t i = 0; i < rounds; ++i, ++n) {
        Rules g;
        switch (r.below(5)) {
        case 0: g = generate(r); break;
        case 1: g = generate_guarded(r); break;
        case 2:
            g = generate_guarded(r);
            mutate(r, g);
            break;
        case 3:
            g = kSeeds[r.below(sizeof(kSeeds) / sizeof(kSeeds[0]))];
            mutate(r, g);
            break;
        default: {
            const size_t rules = 1 + r.below(3);
            for (size_t k = 0; k < rules; ++k) {
                std::string p;
                const size_t len = r.below(24);
                for (size_t j = 0; j < len; ++j) p.push_back(r.coin(2) ? kMeta[r.below(sizeof(kMeta) - 1)] : (char)r.below(256));
                g.emplace_back(kNames[k], p);
            }
        }
        }
        if (!run_one(g, r, tally)) return 1;
    }
    std::printf("grammar_fuzz: %zu grammars, %zu compiled (largest table %zu states), %zu refused; %zu strings walked, %zu to their end, deepest stack %zu; no other outcome\n",
                n, tally.compiled, tally.max_states, tally.refused, tally.walked, tally.survived, tally.deepest);
    return 0;
}
