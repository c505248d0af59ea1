// Draft-model speculative decoding (LlmModel::generate_draft): the small kernels that keep a round -- begin, the drafter's
// passes, the target's verify step -- one chain on the device (draft_model_kernels.hip).  Every model kernel on the chain is
// an existing one; these only move ids and positions between the two models.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kjarni {

struct LlmLookupState;  // llm_kernels.h

// The begin of a round of `rows` (1..8) rows on the target's history T[0, n), n = state->n >= 2 (T[n - 1] is the token that is
// in neither cache): the drafter's position becomes n - 2 and its two input ids T[n - 2], T[n - 1]; the target's ids[0] becomes
// T[n - 1] and ids[1, rows) repeat it until the drafter's picks overwrite them; state->m = rows - 1.  rows == 1 (no drafter
// kernel follows) leaves drafter_ids / drafter_pos alone.  n is clamped to [2, hist_cap] (hist_cap >= 2 entries of T exist; no
// loop produces a history outside that range): nothing is read outside the buffer.
hipError_t launch_draft_begin(const int32_t* history, int hist_cap, LlmLookupState* state, int rows, uint32_t* drafter_ids, int* drafter_pos,
                              uint32_t* ids, hipStream_t stream);

// The hand-off after a drafter pass (two launches): *id_out = argmax(logits[0, vocab)) -- the last maximum wins, launch_argmax's
// rule -- and *drafter_pos += advance.  best_scratch: one zero-initialised u64 (re-zeroed).
hipError_t launch_draft_handoff(const float* logits, int vocab, unsigned long long* best_scratch, uint32_t* id_out, int* drafter_pos,
                                int advance, hipStream_t stream);

}  // namespace kjarni
