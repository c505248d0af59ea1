// Grammar-constrained decoding on the device (gfx950): the stack automaton of grammar.h over a vocabulary.  Which tokens are
// legal depends on the row's stack, so there is no mask made once per state: every step walks every token.
//
//   apply        rows of logits, a device-held GrammarRow per row: where done is clear, each thread walks its token's bytes from
//                the row's configuration; a logit stays as it is when its token has at least one byte and the walk does not die
//                -- or, for one of the call's stop ids, when the configuration is accepted (whatever the stop id's bytes) -- and
//                becomes -inf otherwise.
//   advance      reads each row's picked token and moves that row's state, depth and stack.
//
// A token's own pushes live in a window of kGrammarTokenPushes return states per thread, in LDS; pops below them read the row's
// stack, staged once per workgroup.  A walk that would hold more of its own pushes at once is dead, on the host (Grammar::walk
// with as_token) and here alike.  The kernels reach the tables through one device-resident descriptor, GrammarView, so a captured
// chain holds only the address of the model's own descriptor and serves every grammar written into it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "constraint_kernels.h"
#include "grammar.h"

namespace kjarni {

struct GrammarView {
    const uint32_t* action;   // [states, 256]
    const uint8_t* flags;     // [states]
    const uint32_t* tok_off;  // [vocab + 1]
    const uint8_t* tok_bytes;
    int32_t states, vocab, n_stop, pad;
    uint32_t stops[kConstraintMaxStops];
};

struct GrammarRow {
    uint32_t state;
    int32_t depth, done, violated;
    uint16_t stack[kGrammarMaxDepth];
};

// logits [rows, ld], ld >= vocab; vocab is view->vocab (the grid is sized by it).
hipError_t launch_grammar_apply(float* logits, int64_t ld, int rows, int vocab, const GrammarView* view, const GrammarRow* row_state,
                                hipStream_t stream);
// picked[rows]: where launch_argmax leaves its token.  state_log / depth_log (both null, or both set with rows == 1, count and
// log_cap): the row's state and depth after the step are stored at index *count - 1, the index launch_argmax recorded the pick at.
hipError_t launch_grammar_advance(const int32_t* picked, int rows, const GrammarView* view, GrammarRow* row_state, uint32_t* state_log,
                                  int32_t* depth_log, const int* count, int log_cap, hipStream_t stream);

// A grammar and a token table with their device copies.  Immutable after construction: the configuration of a run belongs to
// the caller.
class DeviceGrammar {
public:
    // Throws InvalidConfig for a malformed table (offsets not monotone / not covering `bytes`) or automaton, before any GPU work.
    DeviceGrammar(int device, Grammar grammar, TokenTable table);
    ~DeviceGrammar();
    DeviceGrammar(const DeviceGrammar&) = delete;
    DeviceGrammar& operator=(const DeviceGrammar&) = delete;

    int device() const { return device_; }
    const Grammar& grammar() const { return grammar_; }
    const TokenTable& table() const { return table_; }
    int vocab() const { return table_.vocab(); }
    // The host's walk of token t from *c, under the rule the kernels keep: false when apply would mask t (no byte, or the walk dies).
    bool step_token(GrammarConfig* c, uint32_t t) const
    {
        return t < (uint32_t)vocab() && table_.length(t) > 0 && grammar_.walk(c, table_.token(t), table_.length(t), true);
    }
    // The descriptor of this grammar with the given stop ids (at most kConstraintMaxStops).
    GrammarView view(const std::vector<uint32_t>& stops) const;
    // The refusal that stands in for DeviceConstraint::check_states.  Configurations are infinitely many, so the rule works on
    // states and over-approximates: a state counts as one a run can be in (reachable()) when it is state 0 or where some token
    // with bytes can end from a reachable state, a walk that pops below the token's own pushes going on in every return state of
    // every call of the rule it leaves (whatever the stack; the depth limit is ignored).  A token is offered in a state when some
    // such walk of it survives.  Throws InvalidConfig naming the first reachable state that offers no token other than a stop id
    // and is either not accepting (nothing can be emitted and the rule cannot end), or accepting in rule 0 with a way on (not
    // no_out) while the call has no stop id to end on.  An accepting state of a called rule passes: its rule can end, and the
    // state below is judged on its own.  What the rule lets through is caught at run time: a row with nothing left picks a masked
    // token, advance sets violated, and the run ends with violated = 1.  Host work only.
    void check_states(const std::vector<uint32_t>& stops) const;
    bool reachable(uint32_t q) const { return q < reachable_.size() && reachable_[q] != 0; }
    uint32_t offered(uint32_t q) const { return q < offered_.size() ? offered_[q] : 0; }  // tokens offered in state q

private:
    int device_;
    Grammar grammar_;
    TokenTable table_;
    std::vector<uint8_t> reachable_;
    std::vector<uint32_t> offered_;
    std::vector<std::vector<uint16_t>> returns_;  // [rule]: the return states of the calls of that rule
    // Walks token t from state q over an unknown stack; the states it can end in are appended to *ends (may be null).  True when any walk survives.
    bool explore(uint32_t q, uint32_t t, std::vector<uint16_t>* ends) const;
    void analyse();
    void* block_ = nullptr;  // action | flags | tok_off | tok_bytes
    uint32_t *action_ = nullptr, *off_ = nullptr;
    uint8_t *flags_ = nullptr, *bytes_ = nullptr;
};

}  // namespace kjarni
