// The pattern parser and Thompson's construction shared by the two host compilers: constraint.cpp (one pattern -> a byte DFA) and
// grammar.cpp (rules of patterns -> a stack automaton).  Internal: plain C++17, included by those two files only.  The one switch
// is Parser::allow_calls: with it, `(?&name)` parses to a Call node (a string of rule `name` here) and the NFA gets an edge over
// that rule's symbol; without it the construct is refused as before.
#pragma once
#include <algorithm>
#include <bitset>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "constraint.h"

namespace kjarni {
namespace regex_detail {

using ByteSet = std::bitset<256>;

constexpr int kMaxDepth = 64;            // nested groups
constexpr size_t kMaxNfaStates = 65536;  // Thompson states ({m,n} copies its operand)
constexpr size_t kMaxRawStates = 16384;  // subset construction, before minimisation
constexpr uint64_t kWorkBudget = 50000000ull;  // closure, subset and refinement steps: a fraction of a second

struct Node {
    enum Kind { Empty, Set, Seq, Alt, Rep, Call } kind = Empty;
    ByteSet set;
    int call = -1;  // Call: index into Parser::calls
    std::vector<int> kids;
    int min = 0, max = 0;  // Rep: max < 0 = unbounded
};

[[noreturn]] inline void fail(const std::string& what, size_t at) { throw ConstraintError("constraint pattern: " + what + " at offset " + std::to_string(at)); }

inline ByteSet range_set(int lo, int hi)
{
    ByteSet s;
    for (int b = lo; b <= hi; ++b) s.set((size_t)b);
    return s;
}

struct Parser {
    const std::string& p;
    size_t i = 0;
    int depth = 0;
    std::vector<Node> nodes;
    bool allow_calls = false;        // (?&name) is a Call node, not a refusal
    std::vector<std::string> calls;  // the distinct names called, in order of first appearance

    explicit Parser(const std::string& pattern, bool with_calls = false) : p(pattern), allow_calls(with_calls) {}

    int add(Node n)
    {
        nodes.push_back(std::move(n));
        return (int)nodes.size() - 1;
    }
    int add_set(const ByteSet& s)
    {
        Node n;
        n.kind = Node::Set;
        n.set = s;
        return add(std::move(n));
    }
    int add_seq(std::vector<int> kids)
    {
        if (kids.size() == 1) return kids[0];
        Node n;
        n.kind = kids.empty() ? Node::Empty : Node::Seq;
        n.kids = std::move(kids);
        return add(std::move(n));
    }
    int add_alt(std::vector<int> kids)
    {
        if (kids.size() == 1) return kids[0];
        Node n;
        n.kind = Node::Alt;
        n.kids = std::move(kids);
        return add(std::move(n));
    }
    int bytes_seq(const uint8_t* b, size_t n)
    {
        std::vector<int> kids;
        for (size_t k = 0; k < n; ++k) kids.push_back(add_set(range_set(b[k], b[k])));
        return add_seq(std::move(kids));
    }
    int ranges_seq(std::initializer_list<std::pair<int, int>> r)
    {
        std::vector<int> kids;
        for (const auto& lh : r) kids.push_back(add_set(range_set(lh.first, lh.second)));
        return add_seq(std::move(kids));
    }
    // `ascii` or any well-formed UTF-8 scalar outside ASCII (no surrogates, no overlong forms, nothing past U+10FFFF)
    int ascii_or_scalar(const ByteSet& ascii)
    {
        std::vector<int> alt;
        if (ascii.any()) alt.push_back(add_set(ascii));
        alt.push_back(ranges_seq({{0xC2, 0xDF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xE0, 0xE0}, {0xA0, 0xBF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xE1, 0xEC}, {0x80, 0xBF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xED, 0xED}, {0x80, 0x9F}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xEE, 0xEF}, {0x80, 0xBF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xF0, 0xF0}, {0x90, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xF1, 0xF3}, {0x80, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}}));
        alt.push_back(ranges_seq({{0xF4, 0xF4}, {0x80, 0x8F}, {0x80, 0xBF}, {0x80, 0xBF}}));
        return add_alt(std::move(alt));
    }

    // One UTF-8 scalar of the pattern at i: its length (the pattern itself must be well formed).
    size_t scalar_len(size_t at) const
    {
        const auto u = [&](size_t k) { return (unsigned)(uint8_t)p[k]; };
        const auto cont = [&](size_t k, unsigned lo, unsigned hi) { return k < p.size() && u(k) >= lo && u(k) <= hi; };
        const unsigned c = u(at);
        if (c < 0x80) return 1;
        if (c >= 0xC2 && c <= 0xDF && cont(at + 1, 0x80, 0xBF)) return 2;
        if (c >= 0xE0 && c <= 0xEF) {
            const unsigned lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
            if (cont(at + 1, lo, hi) && cont(at + 2, 0x80, 0xBF)) return 3;
        }
        if (c >= 0xF0 && c <= 0xF4) {
            const unsigned lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
            if (cont(at + 1, lo, hi) && cont(at + 2, 0x80, 0xBF) && cont(at + 3, 0x80, 0xBF)) return 4;
        }
        fail("invalid UTF-8 in the pattern", at);
    }

    static ByteSet digits() { return range_set('0', '9'); }
    static ByteSet word() { return range_set('0', '9') | range_set('a', 'z') | range_set('A', 'Z') | range_set('_', '_'); }
    static ByteSet space()
    {
        ByteSet s = range_set('\t', '\r');  // \t \n \v \f \r
        s.set(' ');
        return s;
    }

    // The escape whose backslash is at i.  Returns true and a set for \d \w \s; else a single code point below 0x100 in *cp.
    bool escape(ByteSet* set, unsigned* cp)
    {
        const size_t at = i;
        if (i + 1 >= p.size()) fail("trailing backslash", at);
        const unsigned char c = (unsigned char)p[i + 1];
        i += 2;
        switch (c) {
        case 'd': *set = digits(); return true;
        case 'w': *set = word(); return true;
        case 's': *set = space(); return true;
        case 'D': case 'W': case 'S': fail(std::string("unsupported negated shorthand \\") + (char)c, at);
        case 'n': *cp = '\n'; return false;
        case 't': *cp = '\t'; return false;
        case 'r': *cp = '\r'; return false;
        case 'f': *cp = '\f'; return false;
        case 'v': *cp = '\v'; return false;
        case 'A': case 'Z': case 'b': case 'B': fail(std::string("unsupported anchor \\") + (char)c, at);
        case 'u': case 'U': case 'N': fail(std::string("unsupported unicode escape \\") + (char)c, at);
        case 'x': {
            unsigned v = 0;
            for (int k = 0; k < 2; ++k) {
                const int h = i < p.size() ? p[i] : 0;
                int d;
                if (h >= '0' && h <= '9') d = h - '0';
                else if (h >= 'a' && h <= 'f') d = h - 'a' + 10;
                else if (h >= 'A' && h <= 'F') d = h - 'A' + 10;
                else fail("\\x needs two hex digits", at);
                v = v * 16 + (unsigned)d;
                ++i;
            }
            *cp = v;
            return false;
        }
        default: break;
        }
        if (c >= '1' && c <= '9') fail("unsupported back-reference", at);
        if (c == '0') fail("unsupported octal escape", at);
        if (c >= 0x80 || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) fail("unknown escape", at);
        *cp = c;  // an escaped metacharacter or other ASCII punctuation
        return false;
    }

    int code_point_literal(unsigned cp)  // cp < 0x100
    {
        uint8_t b[2];
        if (cp < 0x80) {
            b[0] = (uint8_t)cp;
            return bytes_seq(b, 1);
        }
        b[0] = (uint8_t)(0xC0 | (cp >> 6));
        b[1] = (uint8_t)(0x80 | (cp & 0x3F));
        return bytes_seq(b, 2);
    }

    int parse_class()
    {
        const size_t open = i++;  // '['
        bool negate = false;
        if (i < p.size() && p[i] == '^') {
            negate = true;
            ++i;
        }
        ByteSet members;
        bool first = true;
        for (;;) {
            if (i >= p.size()) fail("unterminated character class", open);
            if (p[i] == ']' && !first) {
                ++i;
                break;
            }
            first = false;
            // one member: a set (\d \w \s) or a single ASCII code point, maybe the low end of a range
            const auto member = [&](ByteSet* set, unsigned* cp) -> bool {
                const size_t at = i;
                if (p[i] == '\\') {
                    const bool is_set = escape(set, cp);
                    if (!is_set && *cp >= 0x80) fail("non-ASCII class member", at);
                    return is_set;
                }
                if ((unsigned char)p[i] >= 0x80) {
                    scalar_len(i);
                    fail("non-ASCII class member", at);
                }
                *cp = (unsigned char)p[i++];
                return false;
            };
            ByteSet set;
            unsigned lo = 0;
            const size_t at = i;
            const bool lo_is_set = member(&set, &lo);
            if (i + 1 < p.size() && p[i] == '-' && p[i + 1] != ']') {
                ++i;
                ByteSet hi_set;
                unsigned hi = 0;
                const bool hi_is_set = member(&hi_set, &hi);
                if (lo_is_set || hi_is_set) fail("bad character range", at);
                if (hi < lo) fail("bad character range (reversed)", at);
                members |= range_set((int)lo, (int)hi);
            } else if (lo_is_set) {
                members |= set;
            } else {
                members.set(lo);
            }
        }
        if (!negate) return add_set(members);
        return ascii_or_scalar(range_set(0, 127) & ~members);
    }

    int parse_atom()
    {
        const size_t at = i;
        const unsigned char c = (unsigned char)p[i];
        switch (c) {
        case '(': {
            ++i;
            if (i < p.size() && p[i] == '?') {
                const char k = i + 1 < p.size() ? p[i + 1] : '\0';
                if (k == ':') i += 2;
                else if (k == '&' && allow_calls) return parse_call(at);
                else if (k == '=' || k == '!') fail("unsupported look-ahead", at);
                else if (k == '<' && i + 2 < p.size() && (p[i + 2] == '=' || p[i + 2] == '!')) fail("unsupported look-behind", at);
                else if (k == 'P' || k == '<') fail("unsupported named group or back-reference", at);
                else if (k == '#') fail("unsupported comment group", at);
                else if (k == '(') fail("unsupported conditional group", at);
                else fail("unsupported inline flags", at);
            }
            if (++depth > kMaxDepth) fail("groups nested deeper than " + std::to_string(kMaxDepth), at);
            const int inner = parse_alt();
            --depth;
            if (i >= p.size() || p[i] != ')') fail("missing ) for the group", at);
            ++i;
            return inner;
        }
        case '[': return parse_class();
        case '.': {
            ++i;
            ByteSet ascii = range_set(0, 127);
            ascii.reset('\n');
            return ascii_or_scalar(ascii);
        }
        case '^': case '$': fail(std::string("unsupported anchor ") + (char)c, at);
        case '*': case '+': case '?': fail("nothing to repeat", at);
        case '{': fail("unsupported construct { (a literal brace is written \\{)", at);
        case '\\': {
            ByteSet set;
            unsigned cp = 0;
            if (escape(&set, &cp)) return add_set(set);
            return code_point_literal(cp);
        }
        default: break;
        }
        const size_t len = scalar_len(i);
        const int node = bytes_seq(reinterpret_cast<const uint8_t*>(p.data()) + i, len);
        i += len;
        return node;
    }

    // (?&name) with i at the '?': a Call node.
    int parse_call(size_t at)
    {
        i += 2;
        const size_t from = i;
        const auto head = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_'; };
        while (i < p.size() && (head(p[i]) || (i > from && p[i] >= '0' && p[i] <= '9'))) ++i;
        if (i == from || i >= p.size() || p[i] != ')') fail("malformed rule call (the form is (?&name), name [A-Za-z_][A-Za-z0-9_]*)", at);
        const std::string name = p.substr(from, i - from);
        ++i;
        size_t k = 0;
        while (k < calls.size() && calls[k] != name) ++k;
        if (k == calls.size()) calls.push_back(name);
        Node n;
        n.kind = Node::Call;
        n.call = (int)k;
        return add(std::move(n));
    }

    // A quantifier at i, if there is one: true and [min, max] (max < 0: unbounded).
    bool quantifier(int* min, int* max)
    {
        if (i >= p.size()) return false;
        const size_t at = i;
        const char c = p[i];
        if (c == '*' || c == '+' || c == '?') {
            *min = c == '+' ? 1 : 0;
            *max = c == '?' ? 1 : -1;
            ++i;
            return true;
        }
        if (c != '{') return false;
        const auto number = [&](int* out) -> bool {
            size_t digits = 0;
            int v = 0;
            while (i < p.size() && p[i] >= '0' && p[i] <= '9') {
                if (++digits > 3) fail("repeat count above 255", at);
                v = v * 10 + (p[i++] - '0');
            }
            *out = v;
            return digits > 0;
        };
        ++i;
        int lo = 0, hi = 0;
        if (!number(&lo)) fail("unsupported construct { (a quantifier is {m}, {m,} or {m,n}; a literal brace is written \\{)", at);
        if (i < p.size() && p[i] == '}') {
            hi = lo;
        } else if (i < p.size() && p[i] == ',') {
            ++i;
            if (!number(&hi)) hi = -1;
            if (i >= p.size() || p[i] != '}') fail("malformed quantifier", at);
        } else {
            fail("malformed quantifier", at);
        }
        ++i;
        if (lo > 255 || hi > 255) fail("repeat count above 255", at);
        if (hi >= 0 && hi < lo) fail("quantifier {m,n} with m > n", at);
        *min = lo;
        *max = hi;
        return true;
    }

    int parse_seq()
    {
        std::vector<int> kids;
        while (i < p.size() && p[i] != '|' && p[i] != ')') {
            int node = parse_atom();
            int min = 0, max = 0;
            if (quantifier(&min, &max)) {
                if (i < p.size()) {
                    if (p[i] == '?') fail("unsupported lazy quantifier", i);
                    if (p[i] == '+') fail("unsupported possessive quantifier", i);
                    if (p[i] == '*' || (p[i] == '{' && i + 1 < p.size() && p[i + 1] >= '0' && p[i + 1] <= '9')) fail("multiple repeat", i);
                }
                Node r;
                r.kind = Node::Rep;
                r.kids = {node};
                r.min = min;
                r.max = max;
                node = add(std::move(r));
            }
            kids.push_back(node);
        }
        return add_seq(std::move(kids));
    }

    int parse_alt()
    {
        std::vector<int> branches;
        branches.push_back(parse_seq());
        while (i < p.size() && p[i] == '|') {
            ++i;
            branches.push_back(parse_seq());
        }
        return add_alt(std::move(branches));
    }

    int parse()
    {
        const int root = parse_alt();
        if (i < p.size()) fail("unbalanced )", i);
        return root;
    }
};

struct Nfa {
    struct State {
        std::vector<int> eps;
        int set = -1, to = -1;  // one byte-set edge
        int call = -1;          // or one edge over a rule's symbol (Parser::calls), also to `to`
    };
    std::vector<State> st;
    std::vector<ByteSet> sets;
    std::map<std::string, int> set_ids;

    int fresh()
    {
        if (st.size() >= kMaxNfaStates)
            throw ConstraintError("constraint pattern: expands to more than " + std::to_string(kMaxNfaStates) + " automaton states");
        st.emplace_back();
        return (int)st.size() - 1;
    }
    int set_id(const ByteSet& s)
    {
        const auto it = set_ids.emplace(s.to_string(), (int)sets.size());
        if (it.second) sets.push_back(s);
        return it.first->second;
    }
    struct Frag {
        int in, out;
    };
    Frag build(const std::vector<Node>& nodes, int id)
    {
        const Node& n = nodes[(size_t)id];
        switch (n.kind) {
        case Node::Empty: {
            const int a = fresh();
            return {a, a};
        }
        case Node::Set: {
            const int a = fresh(), b = fresh();
            st[(size_t)a].set = set_id(n.set);
            st[(size_t)a].to = b;
            return {a, b};
        }
        case Node::Call: {
            const int a = fresh(), b = fresh();
            st[(size_t)a].call = n.call;
            st[(size_t)a].to = b;
            return {a, b};
        }
        case Node::Seq: {
            Frag all = build(nodes, n.kids[0]);
            for (size_t k = 1; k < n.kids.size(); ++k) {
                const Frag f = build(nodes, n.kids[k]);
                st[(size_t)all.out].eps.push_back(f.in);
                all.out = f.out;
            }
            return all;
        }
        case Node::Alt: {
            const int a = fresh(), b = fresh();
            for (int kid : n.kids) {
                const Frag f = build(nodes, kid);
                st[(size_t)a].eps.push_back(f.in);
                st[(size_t)f.out].eps.push_back(b);
            }
            return {a, b};
        }
        case Node::Rep: {
            const int a = fresh();
            int out = a;
            for (int k = 0; k < n.min; ++k) {
                const Frag f = build(nodes, n.kids[0]);
                st[(size_t)out].eps.push_back(f.in);
                out = f.out;
            }
            if (n.max < 0) {
                const int loop = fresh();
                st[(size_t)out].eps.push_back(loop);
                const Frag f = build(nodes, n.kids[0]);
                st[(size_t)loop].eps.push_back(f.in);
                st[(size_t)f.out].eps.push_back(loop);
                return {a, loop};
            }
            const int end = fresh();
            for (int k = n.min; k < n.max; ++k) {
                st[(size_t)out].eps.push_back(end);  // stop here ...
                const Frag f = build(nodes, n.kids[0]);  // ... or take one more
                st[(size_t)out].eps.push_back(f.in);
                out = f.out;
            }
            st[(size_t)out].eps.push_back(end);
            return {a, end};
        }
        }
        return {0, 0};
    }
};

// cls[b]: the class of byte b, two bytes sharing a class iff no set tells them apart.  Returns the number of classes.
inline int byte_classes(const std::vector<ByteSet>& sets, int cls[256])
{
    for (int b = 0; b < 256; ++b) cls[b] = 0;
    int n_cls = 1;
    for (const ByteSet& s : sets) {
        std::map<std::pair<int, bool>, int> split;
        int next[256];
        for (int b = 0; b < 256; ++b) {
            const auto it = split.emplace(std::make_pair(cls[b], s.test((size_t)b)), (int)split.size());
            next[b] = it.first->second;
        }
        for (int b = 0; b < 256; ++b) cls[b] = next[b];
        n_cls = (int)split.size();
    }
    return n_cls;
}

struct Budget {
    uint64_t left = kWorkBudget;
    void spend(uint64_t n)
    {
        if (n > left) throw ConstraintError("constraint pattern: too costly to compile (work budget exceeded)");
        left -= n;
    }
};

}  // namespace regex_detail
}  // namespace kjarni
