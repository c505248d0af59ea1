// Constrained decoding on the device (gfx950): the token mask of a byte DFA (constraint.h) over a vocabulary, the in-place
// logits processor that applies it, and the step that moves the automaton by the picked token.
//
//   mask build   mask[S][ceil(V / 64)] 64-bit words + count[S]: bit (q, t) is set iff token t has at least one byte and walking
//                its bytes from state q never reaches kConstraintDead.  Once per (pattern, vocabulary).
//   apply        rows of logits, a device-held (state, done, violated) per row: where done is clear, a logit stays as it is
//                when its token's bit is set -- or, for one of the call's stop ids, when the state is accepting (a stop id is
//                governed by that rule alone, whatever its bytes) -- and becomes -inf otherwise.
//   advance      reads each row's picked token and moves that row's state.
//
// The kernels reach the tables through one device-resident descriptor, ConstraintView, so a captured chain holds only the
// address of the model's own descriptor and serves every constraint written into it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "constraint.h"

namespace kjarni {

constexpr int kConstraintMaxStops = 16;                      // (include/kjarni_hip.h: KJARNI_CONSTRAINT_MAX_STOPS)
constexpr size_t kConstraintMaxMaskBytes = (size_t)256 << 20;  // a larger mask is refused

struct ConstraintView {
    const unsigned long long* mask;  // [states, words]
    const uint16_t* trans;           // [states, 256]
    const uint8_t* flags;            // [states]: bit 0 accepting, bit 1 closed
    const uint32_t* tok_off;         // [vocab + 1]
    const uint8_t* tok_bytes;
    int32_t states, vocab, words, n_stop;
    uint32_t stops[kConstraintMaxStops];
};

struct ConstraintRow {
    uint32_t state;
    int32_t done, violated, pad;
};

// count[states] must be zero; mask needs no initialisation (every word is stored).
hipError_t launch_constraint_mask(const uint16_t* trans, int states, const uint32_t* tok_off, const uint8_t* tok_bytes, int vocab,
                                  unsigned long long* mask, uint32_t* count, hipStream_t stream);
// logits [rows, ld], ld >= view->vocab; the row width masked is view->vocab.
hipError_t launch_constraint_apply(float* logits, int64_t ld, int rows, int vocab, const ConstraintView* view, const ConstraintRow* row_state,
                                   hipStream_t stream);
// picked[rows]: where launch_argmax leaves its token (LlmModel: token_).  state_log (null, or rows == 1 with count and log_cap): the
// row's state after the step is stored at state_log[*count - 1], the index launch_argmax recorded the pick at.
hipError_t launch_constraint_advance(const int32_t* picked, int rows, const ConstraintView* view, ConstraintRow* row_state, uint32_t* state_log,
                                     const int* count, int log_cap, hipStream_t stream);

// The token table of a vocabulary: token t contributes tok_bytes[tok_off[t], tok_off[t + 1]).
struct TokenTable {
    std::vector<uint32_t> off;   // [vocab + 1]
    std::vector<uint8_t> bytes;
    int vocab() const { return off.empty() ? 0 : (int)off.size() - 1; }
    const uint8_t* token(uint32_t t) const { return bytes.data() + off[t]; }
    size_t length(uint32_t t) const { return off[(size_t)t + 1] - off[t]; }
};

// A DFA and a token table with their mask in device memory.  Immutable after construction: the state of a run belongs to the
// caller (LlmModel keeps it next to its own ConstraintView).
class DeviceConstraint {
public:
    // Throws InvalidConfig for a malformed table (offsets not monotone / not covering `bytes`) and a mask beyond
    // kConstraintMaxMaskBytes, before any GPU work.
    DeviceConstraint(int device, ConstraintDfa dfa, TokenTable table);
    ~DeviceConstraint();
    DeviceConstraint(const DeviceConstraint&) = delete;
    DeviceConstraint& operator=(const DeviceConstraint&) = delete;

    int device() const { return device_; }
    const ConstraintDfa& dfa() const { return dfa_; }
    const TokenTable& table() const { return table_; }
    int vocab() const { return table_.vocab(); }
    int words() const { return (vocab() + 63) / 64; }
    const std::vector<uint32_t>& counts() const { return counts_; }  // allowed tokens per state, as the device counted them
    void mask_row(uint32_t state, uint64_t* words_out) const;        // one state's words, from the device
    // Is token t allowed in state q by the host's walk (what bit (q, t) of the mask says)?
    bool allows(uint32_t q, uint32_t t) const
    {
        return t < (uint32_t)vocab() && table_.length(t) > 0 && dfa_.step(q, table_.token(t), table_.length(t)) != kConstraintDead;
    }
    uint32_t step_token(uint32_t q, uint32_t t) const
    {
        return t < (uint32_t)vocab() ? dfa_.step(q, table_.token(t), table_.length(t)) : (uint32_t)kConstraintDead;
    }
    // The descriptor of this constraint with the given stop ids (at most kConstraintMaxStops).
    ConstraintView view(const std::vector<uint32_t>& stops) const;
    // Every state a run can be in (reachable(): the start state and what the allowed tokens lead to from there) must offer an
    // allowed token that is no stop id, or be accepting with stop ids in the call, or be closed: throws InvalidConfig naming the
    // first state that does not.  Host work only.
    void check_states(const std::vector<uint32_t>& stops) const;
    bool reachable(uint32_t q) const { return q < reachable_.size() && reachable_[q] != 0; }

private:
    int device_;
    ConstraintDfa dfa_;
    TokenTable table_;
    std::vector<uint32_t> counts_;
    std::vector<uint8_t> reachable_;
    void* block_ = nullptr;  // trans | flags | tok_off | tok_bytes | count
    unsigned long long* mask_ = nullptr;
    uint16_t* trans_ = nullptr;
    uint8_t *flags_ = nullptr, *bytes_ = nullptr;
    uint32_t *off_ = nullptr, *count_ = nullptr;
};

}  // namespace kjarni
