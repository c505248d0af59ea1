// Pattern -> byte DFA (constraint.h): a recursive-descent parser into a small syntax tree, Thompson's construction over byte
// sets, the subset construction over classes of bytes no set of the pattern tells apart, removal of the states that cannot
// accept, and Moore's partition refinement.  The input is untrusted text: nesting depth, automaton size and total work are
// bounded, and every bound ends in a ConstraintError.
#include "constraint.h"

#include "regex_nfa.h"

namespace kjarni {

using namespace regex_detail;

ConstraintDfa compile_constraint(const std::string& pattern)
{
    Parser parser(pattern);
    const int root = parser.parse();
    Nfa nfa;
    const Nfa::Frag whole = nfa.build(parser.nodes, root);
    const int accept = whole.out;
    Budget budget;

    // classes of bytes that no set of the pattern tells apart
    int cls[256] = {};
    const int n_cls = byte_classes(nfa.sets, cls);
    std::vector<int> rep((size_t)n_cls, 0);
    for (int b = 255; b >= 0; --b) rep[(size_t)cls[b]] = b;

    // subset construction; a DFA state is the sorted list of its NFA states that carry a byte edge, or are the accept state
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
            if (ns.set >= 0 || s == accept) out.push_back(s);
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
    std::vector<std::vector<int>> raw;  // [state][class] -> state, -1 = no move
    std::vector<int> cur, seeds;
    closure({whole.in}, cur);
    ids.emplace(cur, 0);
    members.push_back(cur);
    for (size_t q = 0; q < members.size(); ++q) {
        raw.emplace_back((size_t)n_cls, -1);
        for (int c = 0; c < n_cls; ++c) {
            seeds.clear();
            const std::vector<int>& from = members[q];  // (re-read: `members` grows below)
            budget.spend(from.size());
            for (int s : from) {
                const Nfa::State& ns = nfa.st[(size_t)s];
                if (ns.set >= 0 && nfa.sets[(size_t)ns.set].test((size_t)rep[(size_t)c])) seeds.push_back(ns.to);
            }
            if (seeds.empty()) continue;
            closure(seeds, cur);
            const auto it = ids.emplace(cur, (int)members.size());
            if (it.second) {
                if (members.size() >= kMaxRawStates)
                    throw ConstraintError("constraint pattern: more than " + std::to_string(kMaxRawStates) +
                                          " states before minimisation (the limit is " + std::to_string(kConstraintMaxStates) + " states)");
                members.push_back(cur);
            }
            raw[q][(size_t)c] = it.first->second;
        }
    }
    const size_t n_raw = members.size();
    std::vector<uint8_t> raw_accept(n_raw, 0);
    for (size_t q = 0; q < n_raw; ++q) raw_accept[q] = std::binary_search(members[q].begin(), members[q].end(), accept) ? 1 : 0;

    // the states that can reach an accepting state (backwards search); every other state is dead
    std::vector<std::vector<int>> preds(n_raw);
    for (size_t q = 0; q < n_raw; ++q)
        for (int c = 0; c < n_cls; ++c)
            if (raw[q][(size_t)c] >= 0) preds[(size_t)raw[q][(size_t)c]].push_back((int)q);
    std::vector<uint8_t> live(n_raw, 0);
    stack.clear();
    for (size_t q = 0; q < n_raw; ++q)
        if (raw_accept[q]) {
            live[q] = 1;
            stack.push_back((int)q);
        }
    while (!stack.empty()) {
        const int q = stack.back();
        stack.pop_back();
        for (int r : preds[(size_t)q])
            if (!live[(size_t)r]) {
                live[(size_t)r] = 1;
                stack.push_back(r);
            }
    }
    if (!live[0]) throw ConstraintError("constraint pattern: the language is empty (no string matches)");
    for (size_t q = 0; q < n_raw; ++q)
        for (int c = 0; c < n_cls; ++c)
            if (raw[q][(size_t)c] >= 0 && !live[(size_t)raw[q][(size_t)c]]) raw[q][(size_t)c] = -1;

    // Moore's refinement over the live states: blocks split until every state of a block moves to the same block on every class
    std::vector<int> block(n_raw, -1);
    for (size_t q = 0; q < n_raw; ++q)
        if (live[q]) block[q] = raw_accept[q];
    size_t n_blocks = 0;
    {
        std::vector<int> sig;
        for (;;) {
            std::map<std::vector<int>, int> seen;
            std::vector<int> next(n_raw, -1);
            for (size_t q = 0; q < n_raw; ++q) {
                if (!live[q]) continue;
                sig.assign(1, block[q]);
                for (int c = 0; c < n_cls; ++c) sig.push_back(raw[q][(size_t)c] < 0 ? -1 : block[(size_t)raw[q][(size_t)c]]);
                budget.spend(sig.size() * 4);
                next[q] = seen.emplace(sig, (int)seen.size()).first->second;
            }
            const bool stable = seen.size() == n_blocks;
            n_blocks = seen.size();
            block.swap(next);
            if (stable) break;
        }
    }
    if (n_blocks > (size_t)kConstraintMaxStates)
        throw ConstraintError("constraint pattern: " + std::to_string(n_blocks) + " states, the limit is " + std::to_string(kConstraintMaxStates));

    // number the blocks breadth first from the start state, bytes in order
    std::vector<int> block_rep(n_blocks, -1);
    for (size_t q = 0; q < n_raw; ++q)
        if (live[q] && block_rep[(size_t)block[q]] < 0) block_rep[(size_t)block[q]] = (int)q;
    std::vector<int> number(n_blocks, -1), order;
    number[(size_t)block[0]] = 0;
    order.push_back(block[0]);
    for (size_t k = 0; k < order.size(); ++k) {
        const int q = block_rep[(size_t)order[k]];
        for (int b = 0; b < 256; ++b) {
            const int t = raw[(size_t)q][(size_t)cls[b]];
            if (t < 0) continue;
            const int tb = block[(size_t)t];
            if (number[(size_t)tb] < 0) {
                number[(size_t)tb] = (int)order.size();
                order.push_back(tb);
            }
        }
    }
    ConstraintDfa dfa;
    const size_t S = order.size();
    dfa.start = 0;
    dfa.trans.assign(S * 256, kConstraintDead);
    dfa.accepting.assign(S, 0);
    dfa.closed.assign(S, 0);
    for (size_t k = 0; k < S; ++k) {
        const int q = block_rep[(size_t)order[k]];
        bool any = false;
        for (int b = 0; b < 256; ++b) {
            const int t = raw[(size_t)q][(size_t)cls[b]];
            if (t < 0) continue;
            dfa.trans[k * 256 + (size_t)b] = (uint16_t)number[(size_t)block[(size_t)t]];
            any = true;
        }
        dfa.accepting[k] = raw_accept[(size_t)q];
        dfa.closed[k] = raw_accept[(size_t)q] && !any;
    }
    return dfa;
}

}  // namespace kjarni
