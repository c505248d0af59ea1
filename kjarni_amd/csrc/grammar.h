// Constrained decoding with a stack, host side: a grammar compiled to a deterministic stack automaton over bytes.  No device
// code and no dependency on the rest of the library (plain C++17), so the compiler can be built alone.
//
// A grammar is a list of rules (name, pattern); rule 0 is the start rule.  A pattern is the syntax of constraint.h plus one
// construct, (?&name): a string of rule `name` here.  The language is the context-free language the rules define, full match
// from rule 0, over bytes, with at most kGrammarMaxDepth calls open at a time (a string that nests deeper is not matched).
//
// Each rule becomes a DFA over bytes and one symbol per called rule; the states of all rules share one numbering, state 0 the
// start state of rule 0.  The machine is one table action[states][256] of 32-bit entries and flags[states]:
//   entry bits 31..30  0 none, 1 move, 2 call
//   move               bits 11..0 the next state
//   call               bits 11..0 the callee's start state, bits 23..12 the state to return to
//   flags bit 0        accepting in its rule;  bit 1  no_out: no byte has a move or a call
// One byte b at (state q, stack of return states, depth d):
//   loop: a = action[q][b]
//         move: q = a.next; done
//         call: d == 64 -> dead;  push a.ret;  q = a.next;  again      (the callee sees the same byte)
//         none: accepting[q] and d > 0 -> q = pop;  again               (the rule ended before this byte)
//               otherwise dead
// The compiler refuses (GrammarError naming the rule) every grammar for which this machine would not recognise exactly the
// grammar's language: see compile_grammar.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "constraint.h"

namespace kjarni {

constexpr int kGrammarMaxRules = 256;     // (include/kjarni_hip.h: KJARNI_GRAMMAR_MAX_RULES)
constexpr int kGrammarMaxStates = 4096;   // (KJARNI_GRAMMAR_MAX_STATES)
constexpr int kGrammarMaxDepth = 64;      // (KJARNI_GRAMMAR_MAX_DEPTH)
constexpr int kGrammarTokenPushes = 16;   // (KJARNI_GRAMMAR_TOKEN_PUSHES)

constexpr uint32_t kGrammarMove = 1u << 30, kGrammarCall = 2u << 30;
constexpr uint8_t kGrammarAccepting = 1, kGrammarNoOut = 2;
// One byte takes at most kGrammarMaxDepth pops and then one chain of first calls (no rule twice: no left recursion).
constexpr int kGrammarMaxByteSteps = kGrammarMaxDepth + kGrammarMaxRules + 2;

// What the C surface reports as InvalidConfig.
using GrammarError = ConstraintError;

// A configuration of the automaton.
struct GrammarConfig {
    uint32_t state = 0;
    int32_t depth = 0;
    uint16_t stack[kGrammarMaxDepth] = {};
};

struct Grammar {
    std::vector<uint32_t> action;   // [states, 256]
    std::vector<uint8_t> flags;     // [states]
    std::vector<uint16_t> rule_of;  // [states]: the rule (numbered as kept, rule 0 first) a state belongs to
    std::vector<std::string> rules; // the names of the rules kept

    int states() const { return (int)flags.size(); }
    bool valid(const GrammarConfig& c) const
    {
        if (c.state >= flags.size() || c.depth < 0 || c.depth > kGrammarMaxDepth) return false;
        for (int i = 0; i < c.depth; ++i)
            if (c.stack[i] >= flags.size()) return false;
        return true;
    }
    // The walk of `n` bytes from *c.  False when it dies (*c is then unspecified) or *c is no configuration of the table.  With
    // as_token, the bytes are one token's: a walk that holds more than kGrammarTokenPushes of its own pushes at once dies (the rule
    // the device kernels keep, so that a token's pushes fit a fixed window).
    bool walk(GrammarConfig* c, const uint8_t* bytes, size_t n, bool as_token) const
    {
        if (!valid(*c)) return false;
        uint32_t q = c->state;
        int d = c->depth, own = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t b = bytes[i];
            for (int steps = 0;; ++steps) {
                if (steps >= kGrammarMaxByteSteps) return false;  // (never with a table from the compiler)
                const uint32_t a = action[(size_t)q * 256 + b];
                if ((a >> 30) == 1) {
                    q = a & 0xFFFu;
                    break;
                }
                if ((a >> 30) == 2) {
                    if (d >= kGrammarMaxDepth || (as_token && own >= kGrammarTokenPushes)) return false;
                    c->stack[d++] = (uint16_t)((a >> 12) & 0xFFFu);
                    ++own;
                    q = a & 0xFFFu;
                    continue;
                }
                if (!(flags[q] & kGrammarAccepting) || d <= 0) return false;
                q = c->stack[--d];
                if (own > 0) --own;
            }
        }
        c->state = q;
        c->depth = d;
        return true;
    }
    bool all_levels(const GrammarConfig& c, uint8_t bit) const
    {
        if (!valid(c) || !(flags[c.state] & bit)) return false;
        for (int i = 0; i < c.depth; ++i)
            if (!(flags[c.stack[i]] & bit)) return false;
        return true;
    }
    bool accepted(const GrammarConfig& c) const { return all_levels(c, kGrammarAccepting); }  // every level is accepting
    bool closed(const GrammarConfig& c) const { return all_levels(c, kGrammarNoOut); }        // every level is no_out
};

// Throws GrammarError, naming the rule (and the byte, where there is one):
//   - every per-pattern refusal of compile_constraint, prefixed with the rule's name;
//   - an undefined name, a duplicate name, a bad name; no rule, more than kGrammarMaxRules rules, more than kGrammarMaxStates
//     states (the message gives the count);
//   - a rule with no finite string; a called rule that matches the empty string; left recursion, direct or through a chain of
//     first calls;
//   - two ways to continue on one byte in one state (a byte edge and the FIRST set of a call, or two calls);
//   - a rule that may either end or go on at a byte that may also follow one of its calls (the LL(1) FIRST/FOLLOW condition,
//     FOLLOW taken through accepting return states, transitively).
// Rules that rule 0 never reaches are parsed (so their own refusals still show) and then dropped.  Total work is bounded.
Grammar compile_grammar(const std::vector<std::pair<std::string, std::string>>& rules);

}  // namespace kjarni
