// A stand-alone driver for the pattern compiler (kjarni_amd/csrc/constraint.cpp), meant to be built with the sanitizers and run
// on the CPU:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ikjarni_amd/csrc \
//       tools/constraint_fuzz.cpp kjarni_amd/csrc/constraint.cpp -o /tmp/constraint_fuzz && /tmp/constraint_fuzz 4000
//
// It feeds the compiler generated patterns (random trees over the whole syntax), mutations of them and of a seed list (bytes
// deleted, duplicated, replaced by metacharacters or by arbitrary bytes), and random byte strings.  Every pattern either compiles
// -- then the table is checked for shape and a few random strings are walked through it -- or ends in a ConstraintError; anything
// else (another exception, a sanitizer report, a crash) fails the run.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "constraint.h"

namespace {

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

const char* const kAtoms[] = {"a", "b", "Z", "0", " ", "\\d", "\\w", "\\s", ".", "\\.", "\\\\", "\\n", "\\t", "\\r", "\\\"", "\\x41", "\\xe9", "\\{", "\\}",
                              "[a-z]", "[^a-z]", "[0-9_]", "[^\"\\\\]", "[\\d\\-x]", "[]a]", "[a-]", "\xC3\xA9", "\xE2\x82\xAC", "\xF0\x9F\x98\x80", "-", "]", "}",
                              ","};
const char* const kQuants[] = {"*", "+", "?", "{0}", "{1}", "{2}", "{3,}", "{0,2}", "{2,5}", "{17}", "{255}", "{0,255}"};
const char* const kSeeds[] = {"-?(?:0|[1-9][0-9]*)", "\"(?:[^\"\\\\\\x00-\\x1f]|\\\\[\"\\\\/bfnrt]|\\\\u[0-9a-fA-F]{4})*\"", "(?:yes|no|maybe)",
                              "\\{\"k\":(?:-?[0-9]+),\"s\":(?:\"[a-z]*\")\\}", "(a|b)*abb", "[ab]*a[ab]{12}", "((((((((a))))))))", "(a?){40}a{40}",
                              "(?:(?:a{10}){10}){10}", "a*?", "^a$", "(?=a)", "(?<=a)b", "(?P<n>a)", "\\1", "a{2,1}", "a{256}", "[z-a]", "[\xC3\xA9]", "(a", "a)",
                              "[a", "\\", "\\x4", "a**", "{", "a{,3}", "\\D", "(?i)a", ".*", "[^a]*", "(.|\\n)*", ""};
const char kMeta[] = "\\.^$*+?{}[]()|-,";

std::string tree(Rng& r, int depth)
{
    const uint32_t pick = r.below(depth <= 0 ? 2 : 8);
    std::string s;
    if (pick < 2) {
        s = kAtoms[r.below(sizeof(kAtoms) / sizeof(kAtoms[0]))];
    } else if (pick < 4) {
        const int n = 1 + (int)r.below(4);
        for (int i = 0; i < n; ++i) s += tree(r, depth - 1);
    } else if (pick < 6) {
        const int n = 2 + (int)r.below(3);
        s = r.coin(2) ? "(?:" : "(";
        for (int i = 0; i < n; ++i) s += (i ? "|" : "") + tree(r, depth - 1);
        s += ")";
    } else {
        s = (r.coin(2) ? "(?:" : "(") + tree(r, depth - 1) + ")";
    }
    if (r.coin(3)) s += kQuants[r.below(sizeof(kQuants) / sizeof(kQuants[0]))];
    return s;
}

std::string mutate(Rng& r, std::string s)
{
    const int edits = 1 + (int)r.below(4);
    for (int e = 0; e < edits; ++e) {
        const size_t at = s.empty() ? 0 : r.below((uint32_t)s.size());
        switch (r.below(5)) {
        case 0:
            if (!s.empty()) s.erase(at, 1 + r.below(3));
            break;
        case 1:
            if (!s.empty()) s.insert(at, s.substr(at, 1 + r.below(6)));
            break;
        case 2: s.insert(at, 1, kMeta[r.below(sizeof(kMeta) - 1)]); break;
        case 3: s.insert(at, 1, (char)r.below(256)); break;
        default:
            if (!s.empty()) s[at] = kMeta[r.below(sizeof(kMeta) - 1)];
            break;
        }
    }
    return s;
}

struct Tally {
    size_t compiled = 0, refused = 0, max_states = 0;
};

bool run_one(const std::string& pattern, Rng& r, Tally& tally)
{
    try {
        const kjarni::ConstraintDfa dfa = kjarni::compile_constraint(pattern);
        const size_t S = (size_t)dfa.states();
        bool ok = S >= 1 && S <= (size_t)kjarni::kConstraintMaxStates && dfa.trans.size() == S * 256 && dfa.closed.size() == S && dfa.start < S;
        bool any_accepting = false;
        for (size_t q = 0; ok && q < S; ++q) {
            bool any = false;
            for (int b = 0; b < 256; ++b) {
                const uint16_t t = dfa.trans[q * 256 + (size_t)b];
                if (t != kjarni::kConstraintDead) {
                    ok = ok && t < S;
                    any = true;
                }
            }
            any_accepting = any_accepting || dfa.accepting[q];
            ok = ok && (dfa.closed[q] != 0) == (dfa.accepting[q] && !any);
        }
        ok = ok && any_accepting;
        if (!ok) {
            std::fprintf(stderr, "malformed table for pattern (%zu bytes): %s\n", pattern.size(), pattern.c_str());
            return false;
        }
        for (int k = 0; k < 4; ++k) {  // walks, with bytes of the pattern itself so that some of them survive
            uint8_t buf[24];
            const size_t n = r.below(sizeof(buf));
            for (size_t i = 0; i < n; ++i) buf[i] = pattern.empty() || r.coin(3) ? (uint8_t)r.below(256) : (uint8_t)pattern[r.below((uint32_t)pattern.size())];
            const uint32_t q = dfa.step(dfa.start, buf, n);
            if (q != kjarni::kConstraintDead && q >= S) {
                std::fprintf(stderr, "step left the table for pattern: %s\n", pattern.c_str());
                return false;
            }
        }
        ++tally.compiled;
        if (S > tally.max_states) tally.max_states = S;
    } catch (const kjarni::ConstraintError&) {
        ++tally.refused;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "unexpected exception '%s' for pattern: %s\n", e.what(), pattern.c_str());
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
    for (const char* seed : kSeeds) {
        ++n;
        if (!run_one(seed, r, tally)) return 1;
    }
    // deep nesting and long inputs, which a recursive parser must bound
    for (const std::string& s : {std::string(5000, '('), std::string(3000, '(') + "a" + std::string(3000, ')'), std::string(20000, 'a'),
                                 std::string(4000, '['), "a" + std::string(3000, '*'), std::string(2000, '|')}) {
        ++n;
        if (!run_one(s, r, tally)) return 1;
    }
    for (size_t i = 0; i < rounds; ++i, ++n) {
        std::string p;
        switch (r.below(4)) {
        case 0: p = tree(r, 1 + (int)r.below(4)); break;
        case 1: p = mutate(r, tree(r, 1 + (int)r.below(4))); break;
        case 2: p = mutate(r, kSeeds[r.below(sizeof(kSeeds) / sizeof(kSeeds[0]))]); break;
        default: {
            const size_t len = r.below(24);
            for (size_t k = 0; k < len; ++k) p.push_back(r.coin(2) ? kMeta[r.below(sizeof(kMeta) - 1)] : (char)r.below(256));
        }
        }
        if (!run_one(p, r, tally)) return 1;
    }
    std::printf("constraint_fuzz: %zu patterns, %zu compiled (largest table %zu states), %zu refused, no other outcome\n", n, tally.compiled,
                tally.max_states, tally.refused);
    return 0;
}
