// Constrained decoding, host side: a regular expression compiled to a DFA over bytes.  No device code and no dependency on
// the rest of the library (plain C++17), so the compiler can be built alone.
//
// Syntax: literals (non-ASCII ones match as their UTF-8 bytes), the escapes \\ \. \n \t \r \f \v \" \xHH and escaped
// metacharacters, \d \w \s with their ASCII meaning, `.` (any Unicode scalar except \n), classes [a-z0-9_] and negated classes
// [^...] over ASCII members, groups ( ) and (?: ), alternation, and the greedy quantifiers * + ? {m} {m,} {m,n} with n <= 255.
// `.` and a negated class also match every well-formed non-ASCII UTF-8 scalar.  The match is a full match: the semantics are
// those of Python's re.fullmatch(pattern, text, re.ASCII) on str, compared on text.encode().  Anchors, lazy and possessive
// quantifiers, back-references, look-around, named groups, inline flags, the negated shorthands and non-ASCII class members are
// refused with a ConstraintError that names the construct and its byte offset in the pattern.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace kjarni {

constexpr uint16_t kConstraintDead = 0xFFFF;  // (include/kjarni_hip.h: KJARNI_CONSTRAINT_DEAD)
constexpr int kConstraintMaxStates = 4096;    // (KJARNI_CONSTRAINT_MAX_STATES)

// What the C surface reports as InvalidConfig.
struct ConstraintError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// The minimal DFA of the pattern's language with the states that cannot reach an accepting state removed: a transition into
// one of those is kConstraintDead.  State 0 is the start state.
struct ConstraintDfa {
    std::vector<uint16_t> trans;      // [states, 256]
    std::vector<uint8_t> accepting;   // [states]
    std::vector<uint8_t> closed;      // [states]: accepting, and every outgoing byte is dead
    uint32_t start = 0;

    int states() const { return (int)accepting.size(); }
    // The state after `n` bytes from `state`; kConstraintDead when the walk dies, or when `state` is no state of the table.
    uint32_t step(uint32_t state, const uint8_t* bytes, size_t n) const
    {
        for (size_t i = 0; i < n; ++i) {
            if (state >= accepting.size()) return kConstraintDead;
            state = trans[(size_t)state * 256 + bytes[i]];
        }
        return state < accepting.size() ? state : (uint32_t)kConstraintDead;
    }
};

// Throws ConstraintError: an unsupported or malformed construct (named, with its offset), more than kConstraintMaxStates
// states (the message gives the count), an empty language.
ConstraintDfa compile_constraint(const std::string& pattern);

}  // namespace kjarni
