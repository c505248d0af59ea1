// Constrained decoding in the lanes (gfx950): a pattern (constraint_kernels.h) or a grammar (grammar_kernels.h) per lane, up to 64
// lanes in one launch, each lane with its own tables, stop ids and row state.
//
//   table     LaneAutomatonTable, device-resident, one slot per lane of either lane set (LlmLaneState: 8, LlmWideState: 64).  Slot l
//             holds the kind of the request in lane l (none / pattern / grammar), that request's ConstraintView or GrammarView (its
//             stop ids inside, as DeviceConstraint::view / DeviceGrammar::view build it) and the lane's ConstraintRow / GrammarRow.
//             A captured chain holds the table's address alone, so one chain per (lane set, width) serves every mix of requests.
//   apply     rows of logits, a lane per blockIdx.y: the mask of constraint_apply_kernel or the walk of grammar_apply_kernel from the
//             lane's own slot, rule for rule (an allowed logit is not rewritten, a stop id is governed by accepting / accepted alone,
//             everything else becomes -inf).  Nothing is written for a frozen lane (live == 0), a lane of kind none, a done row.
//             The logits are rewritten in place, as generate() does: the lanes' pick (argmax_partial_kernel, the one tie rule)
//             then runs unchanged on the masked rows, and the log-probability records read the raw row in a pass ahead of the mask.
//   advance   launched right behind the lanes' pick, one thread per lane.  A lane was live at that pick exactly when its count
//             moved past what the slot has walked; the thread then walks the picked token (the lane's newest history entry) from
//             the lane's row as constraint_advance_kernel / grammar_advance_kernel do.  A stop id in an accepting state (accepted
//             configuration) sets done; a closed state (configuration) sets done and clears live[l] -- the token stays in the
//             history and nothing more is fed; a dead walk sets violated and done and clears live[l].  The limit, the full cache
//             and the token hand-over stay the pick's.  fresh[l] / picked[l] say whether the lane picked and what, for the
//             records' finish pass behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "constraint_kernels.h"
#include "grammar_kernels.h"
#include "llm_kernels.h"

namespace kjarni {

constexpr int kLaneAutomatonSlots = kMaxWideLanes;
constexpr int32_t kLaneKindNone = 0, kLaneKindPattern = 1, kLaneKindGrammar = 2;

struct LaneAutomatonSlot {
    int32_t kind;
    int32_t walked;  // picks of the lane's request the advance has seen (the lane's count between two steps)
    int32_t pad[2];
    ConstraintView cview;  // kind 1
    GrammarView gview;     // kind 2
    ConstraintRow crow;
    GrammarRow grow;
};

struct LaneAutomatonTable {
    LaneAutomatonSlot slot[kLaneAutomatonSlots];
    int32_t fresh[kLaneAutomatonSlots];   // 1: the last advance found a new pick in the lane (it was live at that pick)
    int32_t picked[kLaneAutomatonSlots];  // ... that pick
};

// logits [first_lane + lanes, ld], ld >= vocab; lanes [first_lane, first_lane + lanes) of table and live (the lane state's array,
// device memory).  Every view of the launch must be over `vocab` tokens.
hipError_t launch_lane_automaton_apply(float* logits, int64_t ld, int vocab, int lanes, int first_lane, const LaneAutomatonTable* table,
                                       const int32_t* live, hipStream_t stream);
// Behind a pick over the same lanes: live / count are the lane state's arrays, history [., hist_stride] the pick's.
hipError_t launch_lane_automaton_advance(LaneAutomatonTable* table, int lanes, int first_lane, int32_t* live, const int32_t* count,
                                         const int32_t* history, int hist_stride, hipStream_t stream);
// launch_lane_pick, then the advance: the constrained pick of either state layout.
hipError_t launch_lane_automaton_pick(const float* logits, int64_t ld, int vocab, int lanes, int first_lane, unsigned long long* best_scratch,
                                      LaneStateRef state, int32_t* history, int hist_stride, int capacity, int advance,
                                      LaneAutomatonTable* table, hipStream_t stream);

}  // namespace kjarni
