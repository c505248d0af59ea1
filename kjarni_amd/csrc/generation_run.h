// GenerationRun: the host-side bookkeeping of one generation request (generator.rs:228-381), stated once for every loop of
// LlmModel -- generate(), generate_lanes(), generate_lookup() and generate_lookup_sampled().  No device code: plain C++17.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "sampling.h"

namespace kjarni {

class DeviceConstraint;  // constraint_kernels.h
class DeviceGrammar;     // grammar_kernels.h

// How a constrained run ended (LlmModel::generate with GenerateOptions::constraint or ::grammar; under a grammar "state" reads
// "configuration": accepted = every level accepting, closed = every level without a way on).
struct ConstraintOutcome {
    uint32_t final_state = 0;   // the automaton's state after the emitted tokens, as the host walked it
    uint32_t device_state = 0;  // ... and as the device held it after the last emitted token (the host checker path: the host's)
    bool accepted = false;      // final_state is accepting
    bool complete = false;      // the run ended on a stop id in an accepting state, or in a closed state
    bool violated = false;      // a token outside the mask was picked (never, for finite logits)
    int32_t final_depth = 0, device_depth = 0;  // under a grammar: the stack depths that go with the two states
};

// The log-probability records of a run (GenerateOptions::logprobs), one per emitted token, in emission order.
struct TokenLogprobs {
    int top_k = 0;
    std::vector<float> logprob;        // [tokens]: the emitted token's log-probability
    std::vector<uint32_t> topk_ids;    // [tokens, top_k]: the most likely tokens, score_topk's order
    std::vector<float> topk_logprob;   // [tokens, top_k]
    void clear(int k)
    {
        top_k = k;
        logprob.clear();
        topk_ids.clear();
        topk_logprob.clear();
    }
    // ids / lps: at least top_k entries
    void push(float lp, const uint32_t* ids, const float* lps)
    {
        logprob.push_back(lp);
        topk_ids.insert(topk_ids.end(), ids, ids + top_k);
        topk_logprob.insert(topk_logprob.end(), lps, lps + top_k);
    }
};

// One run of run_generation_loop (generator.rs:228-381).
struct GenerateOptions {
    size_t max_new_tokens = 0;
    size_t max_len = 0;  // prompt + generated cap (generator.rs:243-246); 0 = prompt + max_new_tokens
    float repetition_penalty = 1.0f;
    int no_repeat_ngram = 0;
    bool sample = false;  // DecodingStrategy::Sample(params) instead of Greedy
    SamplingParams sampling;
    std::vector<uint32_t> stop_ids;  // empty: every eos_token_id of config.json
    std::function<float()> uniform;  // the draw in [0, 1) for each sampled token
    // Constrained decoding: generate() takes it, and the lanes per request (generate_lanes / generate_wide); the lookup and draft
    // entry points refuse it.
    const DeviceConstraint* constraint = nullptr;
    ConstraintOutcome* constraint_outcome = nullptr;  // may be null
    // ... or a grammar (a stack automaton: grammar_kernels.h) in its place; setting both is InvalidConfig.  The outcome as above.
    const DeviceGrammar* grammar = nullptr;
    // Log-probabilities of the emitted tokens (logprob_kernels.h): -1 = off (nothing changes: the same graphs, the same launches),
    // 0 .. KJARNI_SCORE_TOPK_MAX = the emitted token's logprob and that many alternatives, under the log-softmax of the logits as
    // the vocabulary head wrote them (before the mask, the processors, temperature and the cut).  generate() alone takes it; the
    // lookup and draft loops forward a request that sets it to generate() (stats zero, the drafter untouched).
    int logprobs = -1;
    TokenLogprobs* logprob_sink = nullptr;  // cleared, then one record per emitted token; may be null
};

// What a loop does with the last token of a run that ends on max_new_tokens.  The choice shows in the cache length a call
// leaves, so each loop names the one it takes.
enum class LastToken {
    Fed,     // one more step runs on it: the cache ends at prompt + max_new_tokens rows
    NotFed,  // the run ends where the token was decided: the cache ends one row short of it
};

struct GenerationRun {
    std::vector<uint32_t> all;           // prompt + emitted tokens
    std::vector<uint32_t>* out = nullptr;  // where the emitted tokens go (the caller's vector)
    std::vector<uint32_t> stops;         // the request's stop ids, or the model's when it names none
    size_t context_limit = 0;            // generator.rs:243-246 and 309-317: the capacity and max_len = prompt + max_new_tokens | max_length
    size_t max_new = 0;
    bool done = true;                    // nothing more is emitted: a stop id, a limit met by accept(), or the callback
    bool cancelled = false;              // ... it was the callback

    GenerationRun() = default;
    GenerationRun(const std::vector<uint32_t>& prompt, const GenerateOptions& opt, size_t capacity, const std::vector<uint32_t>& default_stops,
                  std::vector<uint32_t>& out_)
        : all(prompt), out(&out_), stops(opt.stop_ids.empty() ? default_stops : opt.stop_ids),
          context_limit(std::min(capacity, opt.max_len ? opt.max_len : prompt.size() + opt.max_new_tokens)), max_new(opt.max_new_tokens),
          done(opt.max_new_tokens == 0)
    {
    }

    bool is_stop(uint32_t t) const { return std::find(stops.begin(), stops.end(), t) != stops.end(); }
    // May another token be decided?  A sampled loop asks before it takes a draw.
    bool wants_token() const { return !done && out->size() < max_new && all.size() < context_limit; }
    // Tokens the run may still emit if no stop id or callback ends it (what a lane's device-side limit is set to).
    size_t tokens_left() const { return wants_token() ? std::min(max_new - out->size(), context_limit - all.size()) : 0; }

    // The drain: `tok` joins `all` and the output unless the run is at a limit or `tok` is a stop id (false: nothing was emitted,
    // the run is done); then on_token (false ends the run), then the max_new_tokens check.
    bool accept(uint32_t tok, const std::function<bool(uint32_t)>& on_token)
    {
        if (!wants_token() || is_stop(tok)) {
            done = true;
            return false;
        }
        all.push_back(tok);
        out->push_back(tok);
        if (on_token && !on_token(tok)) done = cancelled = true;
        if (out->size() >= max_new) done = true;
        return true;
    }

    // After accept(): is the token it took the input of another step?  Never once the callback said stop or the context is
    // full, nor when accept() refused the token (LastToken::NotFed answers that by itself: the run is done; a LastToken::Fed
    // loop asks only after accept() returned true); the last token of max_new_tokens as `last` says.  With max_len = 0 that
    // token also fills context_limit = prompt + max_new_tokens, so Fed and NotFed differ only under an explicit larger max_len.
    // (The loops whose device feeds itself -- plain greedy, the lookup loops, the captured lane step -- do not ask: their
    // bursts are sized by what is left.)
    bool feeds_accepted(LastToken last) const
    {
        if (cancelled || all.size() >= context_limit) return false;
        return !done || last == LastToken::Fed;
    }
};

}  // namespace kjarni
