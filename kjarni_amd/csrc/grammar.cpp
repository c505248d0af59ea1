// Grammar -> stack automaton (grammar.h).  Every rule goes through the parser and Thompson's construction of the pattern
// compiler (regex_nfa.h, with the rule-call switch on) and a subset construction over the rule's byte classes plus one symbol per
// called rule.  The rules are then judged together: reachability from rule 0, productivity, empty callees, left recursion, FIRST
// and FOLLOW sets, and the two determinism conditions.  What passes is numbered and written as one action table.  The input is
// untrusted: one work budget covers all rules, and every bound ends in a GrammarError.
#include "grammar.h"

#include <cstdio>

#include "regex_nfa.h"

namespace kjarni {

using namespace regex_detail;

namespace {

struct RuleDfa {
    std::string name;
    std::vector<int> call_rule;                             // the parser's call index -> rule index
    int cls[256] = {};
    int n_cls = 1;
    std::vector<std::vector<int>> byte_to;                  // [state][class] -> state, -1 none
    std::vector<std::vector<std::pair<int, int>>> call_to;  // [state] -> (rule, state), one per called rule
    std::vector<uint8_t> accept;
    std::vector<uint8_t> live;
    std::vector<ByteSet> byte_out, out;                     // [state]: the bytes with a byte edge; with any way on
    size_t states() const { return accept.size(); }
};

[[noreturn]] void refuse(const std::string& rule, const std::string& what) { throw GrammarError("grammar rule '" + rule + "': " + what); }

std::string byte_name(int b)
{
    char buf[32];
    if (b > 0x20 && b < 0x7F) std::snprintf(buf, sizeof(buf), "0x%02x ('%c')", b, b);
    else std::snprintf(buf, sizeof(buf), "0x%02x", b);
    return buf;
}

int first_bit(const ByteSet& s)
{
    for (int b = 0; b < 256; ++b)
        if (s.test((size_t)b)) return b;
    return -1;
}

bool good_name(const std::string& n)
{
    if (n.empty() || n.size() > 255) return false;
    for (size_t i = 0; i < n.size(); ++i) {
        const char c = n[i];
        const bool head = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_';
        if (!head && !(i > 0 && c >= '0' && c <= '9')) return false;
    }
    return true;
}

// One rule's pattern -> its DFA over byte classes and call symbols (calls still named by the parser's index).
void build_rule(const std::string& pattern, RuleDfa& r, std::vector<std::string>& called, Budget& budget)
{
    Parser parser(pattern, true);
    const int root = parser.parse();
    Nfa nfa;
    const Nfa::Frag whole = nfa.build(parser.nodes, root);
    const int accept = whole.out;
    called = parser.calls;
    const int n_calls = (int)called.size();
    r.n_cls = byte_classes(nfa.sets, r.cls);
    std::vector<int> rep((size_t)r.n_cls, 0);
    for (int b = 255; b >= 0; --b) rep[(size_t)r.cls[b]] = b;

    std::vector<uint32_t> stamp(nfa.st.size(), 0);
    uint32_t generation = 0;
    std::vector<int> stack;
    const auto closure = [&](const std::vector<int>& seeds, std::vector<int>& out) {
        out.clear();
        ++generation;
        stack.clear();
        for (int s : seeds)
            if (stamp[(size_t)s] != generation) {
                stamp[(size_t)s] = generation;
                stack.push_back(s);
            }
        while (!stack.empty()) {
            const int s = stack.back();
            stack.pop_back();
            const Nfa::State& ns = nfa.st[(size_t)s];
            if (ns.set >= 0 || ns.call >= 0 || s == accept) out.push_back(s);
            budget.spend(1 + ns.eps.size());
            for (int t : ns.eps)
                if (stamp[(size_t)t] != generation) {
                    stamp[(size_t)t] = generation;
                    stack.push_back(t);
                }
        }
        std::sort(out.begin(), out.end());
    };
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<int>> members;
    std::vector<int> cur, seeds;
    closure({whole.in}, cur);
    ids.emplace(cur, 0);
    members.push_back(cur);
    const auto target = [&]() -> int {
        closure(seeds, cur);
        const auto it = ids.emplace(cur, (int)members.size());
        if (it.second) {
            if (members.size() >= kMaxRawStates)
                throw ConstraintError("more than " + std::to_string(kMaxRawStates) + " states in one rule (the limit is " +
                                      std::to_string(kGrammarMaxStates) + " states for the whole grammar)");
            members.push_back(cur);
        }
        return it.first->second;
    };
    for (size_t q = 0; q < members.size(); ++q) {
        r.byte_to.emplace_back((size_t)r.n_cls, -1);
        r.call_to.emplace_back();
        for (int c = 0; c < r.n_cls + n_calls; ++c) {
            seeds.clear();
            const std::vector<int>& from = members[q];  // (re-read: `members` grows below)
            budget.spend(from.size());
            for (int s : from) {
                const Nfa::State& ns = nfa.st[(size_t)s];
                if (c < r.n_cls ? (ns.set >= 0 && nfa.sets[(size_t)ns.set].test((size_t)rep[(size_t)c])) : ns.call == c - r.n_cls) seeds.push_back(ns.to);
            }
            if (seeds.empty()) continue;
            const int t = target();
            if (c < r.n_cls) r.byte_to[q][(size_t)c] = t;
            else r.call_to[q].emplace_back(c - r.n_cls, t);  // (the parser's index for now)
        }
    }
    r.accept.resize(members.size());
    for (size_t q = 0; q < members.size(); ++q) r.accept[q] = std::binary_search(members[q].begin(), members[q].end(), accept) ? 1 : 0;
}

}  // namespace

Grammar compile_grammar(const std::vector<std::pair<std::string, std::string>>& rules)
{
    if (rules.empty()) throw GrammarError("grammar: no rule (rule 0 is the start rule)");
    if (rules.size() > (size_t)kGrammarMaxRules)
        throw GrammarError("grammar: " + std::to_string(rules.size()) + " rules, the limit is " + std::to_string(kGrammarMaxRules));
    const int R = (int)rules.size();
    std::map<std::string, int> index;
    for (int r = 0; r < R; ++r) {
        if (!good_name(rules[(size_t)r].first)) throw GrammarError("grammar: bad rule name at rule " + std::to_string(r) + " (a name is [A-Za-z_][A-Za-z0-9_]*)");
        if (!index.emplace(rules[(size_t)r].first, r).second) refuse(rules[(size_t)r].first, "defined twice");
    }
    Budget budget;
    std::vector<RuleDfa> dfa((size_t)R);
    std::vector<std::vector<std::string>> called((size_t)R);
    for (int r = 0; r < R; ++r) {
        dfa[(size_t)r].name = rules[(size_t)r].first;
        try {
            build_rule(rules[(size_t)r].second, dfa[(size_t)r], called[(size_t)r], budget);
        } catch (const ConstraintError& e) {
            refuse(dfa[(size_t)r].name, e.what());
        }
    }
    for (int r = 0; r < R; ++r) {
        RuleDfa& d = dfa[(size_t)r];
        for (const std::string& n : called[(size_t)r]) {
            const auto it = index.find(n);
            if (it == index.end()) refuse(d.name, "calls the undefined rule '" + n + "'");
            d.call_rule.push_back(it->second);
        }
        for (auto& edges : d.call_to)
            for (auto& e : edges) e.first = d.call_rule[(size_t)e.first];
    }

    // the rules rule 0 reaches through calls
    std::vector<uint8_t> reached((size_t)R, 0);
    std::vector<int> todo = {0};
    reached[0] = 1;
    while (!todo.empty()) {
        const int r = todo.back();
        todo.pop_back();
        for (int c : dfa[(size_t)r].call_rule)
            if (!reached[(size_t)c]) {
                reached[(size_t)c] = 1;
                todo.push_back(c);
            }
    }

    // productivity: a state is live when it accepts, or moves to a live state, or calls a productive rule and returns to a live
    // state; a rule is productive when its start state is live
    std::vector<uint8_t> productive((size_t)R, 0);
    for (int r = 0; r < R; ++r) dfa[(size_t)r].live.assign(dfa[(size_t)r].states(), 0);
    for (bool changed = true; changed;) {
        changed = false;
        for (int r = 0; r < R; ++r) {
            if (!reached[(size_t)r]) continue;
            RuleDfa& d = dfa[(size_t)r];
            for (size_t q = d.states(); q-- > 0;) {
                if (d.live[q]) continue;
                budget.spend((uint64_t)d.n_cls + d.call_to[q].size() + 1);
                bool live = d.accept[q] != 0;
                for (int c = 0; c < d.n_cls && !live; ++c) live = d.byte_to[q][(size_t)c] >= 0 && d.live[(size_t)d.byte_to[q][(size_t)c]];
                for (const auto& e : d.call_to[q]) live = live || (productive[(size_t)e.first] && d.live[(size_t)e.second]);
                if (live) {
                    d.live[q] = 1;
                    changed = true;
                }
            }
            if (d.live[0] && !productive[(size_t)r]) {
                productive[(size_t)r] = 1;
                changed = true;
            }
        }
    }
    for (int r = 0; r < R; ++r)
        if (reached[(size_t)r] && !productive[(size_t)r]) refuse(dfa[(size_t)r].name, "no finite string matches the rule");
    for (int r = 0; r < R; ++r) {  // trim: nothing leads into a state that cannot reach the rule's end
        if (!reached[(size_t)r]) continue;
        RuleDfa& d = dfa[(size_t)r];
        for (size_t q = 0; q < d.states(); ++q) {
            for (int c = 0; c < d.n_cls; ++c)
                if (d.byte_to[q][(size_t)c] >= 0 && !d.live[(size_t)d.byte_to[q][(size_t)c]]) d.byte_to[q][(size_t)c] = -1;
            auto& edges = d.call_to[q];
            edges.erase(std::remove_if(edges.begin(), edges.end(), [&](const std::pair<int, int>& e) { return !d.live[(size_t)e.second]; }), edges.end());
        }
    }

    // a called rule must not match the empty string (the callee always takes the byte it was called on)
    for (int r = 0; r < R; ++r) {
        if (!reached[(size_t)r]) continue;
        for (size_t q = 0; q < dfa[(size_t)r].states(); ++q)
            for (const auto& e : dfa[(size_t)r].call_to[q])
                if (dfa[(size_t)e.first].accept[0])
                    refuse(dfa[(size_t)e.first].name, "matches the empty string and is called (by rule '" + dfa[(size_t)r].name + "')");
    }

    // left recursion: a cycle among the calls made in start states; FIRST sets along the way (depth-first, callees first)
    std::vector<ByteSet> first((size_t)R);
    std::vector<uint8_t> colour((size_t)R, 0);  // 1 on the path, 2 finished
    {
        struct Frame {
            int rule;
            size_t edge;
        };
        std::vector<Frame> path;
        for (int root = 0; root < R; ++root) {
            if (!reached[(size_t)root] || colour[(size_t)root]) continue;
            path.push_back({root, 0});
            colour[(size_t)root] = 1;
            while (!path.empty()) {
                Frame& f = path.back();
                const RuleDfa& d = dfa[(size_t)f.rule];
                budget.spend(1);
                if (f.edge < d.call_to[0].size()) {
                    const int c = d.call_to[0][f.edge++].first;
                    if (colour[(size_t)c] == 1) refuse(dfa[(size_t)c].name, "left recursion (the rule calls itself before taking a byte, directly or through other rules)");
                    if (colour[(size_t)c] == 0) {
                        colour[(size_t)c] = 1;
                        path.push_back({c, 0});
                    }
                    continue;
                }
                ByteSet s;
                for (int b = 0; b < 256; ++b)
                    if (d.byte_to[0][(size_t)d.cls[b]] >= 0) s.set((size_t)b);
                for (const auto& e : d.call_to[0]) s |= first[(size_t)e.first];
                first[(size_t)f.rule] = s;
                colour[(size_t)f.rule] = 2;
                path.pop_back();
            }
        }
    }

    // one way to continue per state and byte
    for (int r = 0; r < R; ++r) {
        if (!reached[(size_t)r]) continue;
        RuleDfa& d = dfa[(size_t)r];
        d.byte_out.assign(d.states(), ByteSet());
        d.out.assign(d.states(), ByteSet());
        for (size_t q = 0; q < d.states(); ++q) {
            budget.spend(256);
            ByteSet s;
            for (int b = 0; b < 256; ++b)
                if (d.byte_to[q][(size_t)d.cls[b]] >= 0) s.set((size_t)b);
            d.byte_out[q] = s;
            for (const auto& e : d.call_to[q]) {
                const ByteSet both = s & first[(size_t)e.first];
                if (both.any()) {
                    const std::string other = (d.byte_out[q] & both).any() ? "a byte edge of the rule's own" : "the start of another called rule";
                    refuse(d.name, "two ways to continue on byte " + byte_name(first_bit(both)) + ": " + other + " and the start of rule '" +
                                       dfa[(size_t)e.first].name + "'");
                }
                s |= first[(size_t)e.first];
            }
            d.out[q] = s;
        }
    }

    // FOLLOW: what may come after a string of the rule, through accepting return states, transitively
    std::vector<ByteSet> follow((size_t)R);
    for (bool changed = true; changed;) {
        changed = false;
        for (int r = 0; r < R; ++r) {
            if (!reached[(size_t)r]) continue;
            const RuleDfa& d = dfa[(size_t)r];
            for (size_t q = 0; q < d.states(); ++q)
                for (const auto& e : d.call_to[q]) {
                    budget.spend(4);
                    ByteSet s = follow[(size_t)e.first] | d.out[(size_t)e.second];
                    if (d.accept[(size_t)e.second]) s |= follow[(size_t)r];
                    if (s != follow[(size_t)e.first]) {
                        follow[(size_t)e.first] = s;
                        changed = true;
                    }
                }
        }
    }
    for (int r = 0; r < R; ++r) {
        if (!reached[(size_t)r]) continue;
        const RuleDfa& d = dfa[(size_t)r];
        for (size_t q = 0; q < d.states(); ++q) {
            const ByteSet both = d.out[q] & follow[(size_t)r];
            if (d.accept[q] && both.any())
                refuse(d.name, "may either end or go on at byte " + byte_name(first_bit(both)) + ", which may also follow a call of the rule");
        }
    }

    // numbering: rule 0 first, the other kept rules in the order given; within a rule breadth first from its start state
    std::vector<int> kept;
    for (int r = 0; r < R; ++r)
        if (reached[(size_t)r]) kept.push_back(r);
    std::vector<std::vector<int>> number((size_t)R), order((size_t)R);
    std::vector<size_t> base((size_t)R, 0);
    size_t total = 0;
    for (int r : kept) {
        const RuleDfa& d = dfa[(size_t)r];
        std::vector<int>& num = number[(size_t)r];
        std::vector<int>& ord = order[(size_t)r];
        num.assign(d.states(), -1);
        num[0] = 0;
        ord.push_back(0);
        const auto visit = [&](int t) {
            if (t >= 0 && num[(size_t)t] < 0) {
                num[(size_t)t] = (int)ord.size();
                ord.push_back(t);
            }
        };
        for (size_t k = 0; k < ord.size(); ++k) {
            const int q = ord[k];
            budget.spend(256);
            for (int b = 0; b < 256; ++b) visit(d.byte_to[(size_t)q][(size_t)d.cls[b]]);
            for (const auto& e : d.call_to[(size_t)q]) visit(e.second);
        }
        base[(size_t)r] = total;
        total += ord.size();
    }
    if (total > (size_t)kGrammarMaxStates)
        throw GrammarError("grammar: " + std::to_string(total) + " states, the limit is " + std::to_string(kGrammarMaxStates));

    Grammar g;
    g.action.assign(total * 256, 0);
    g.flags.assign(total, 0);
    g.rule_of.assign(total, 0);
    for (size_t k = 0; k < kept.size(); ++k) {
        const int r = kept[k];
        const RuleDfa& d = dfa[(size_t)r];
        g.rules.push_back(d.name);
        for (size_t i = 0; i < order[(size_t)r].size(); ++i) {
            const int q = order[(size_t)r][i];
            const size_t at = base[(size_t)r] + i;
            g.rule_of[at] = (uint16_t)k;
            g.flags[at] = (uint8_t)((d.accept[(size_t)q] ? kGrammarAccepting : 0) | (d.out[(size_t)q].none() ? kGrammarNoOut : 0));
            for (int b = 0; b < 256; ++b) {
                const int t = d.byte_to[(size_t)q][(size_t)d.cls[b]];
                if (t >= 0) {
                    g.action[at * 256 + (size_t)b] = kGrammarMove | (uint32_t)(base[(size_t)r] + (size_t)number[(size_t)r][(size_t)t]);
                    continue;
                }
                for (const auto& e : d.call_to[(size_t)q])
                    if (first[(size_t)e.first].test((size_t)b))
                        g.action[at * 256 + (size_t)b] = kGrammarCall | (uint32_t)((base[(size_t)r] + (size_t)number[(size_t)r][(size_t)e.second]) << 12) |
                                                         (uint32_t)base[(size_t)e.first];
            }
        }
    }
    return g;
}

}  // namespace kjarni
