// Constrained decoding in the lanes, kernels for gfx950 (lane_constraint_kernels.h).
#include "lane_constraint_kernels.h"

#include <cmath>

namespace kjarni {

namespace {

constexpr int kApplyThreads = 256, kAdvanceThreads = kLaneAutomatonSlots;
constexpr uint8_t kFlagAccepting = 1, kFlagClosed = 2;  // ConstraintView::flags (constraint_kernels.hip)

__device__ __forceinline__ bool lane_is_stop(const uint32_t* stops, int n, uint32_t v)
{
    bool stop = false;
    for (int i = 0; i < n && i < kConstraintMaxStops; ++i) stop |= stops[i] == v;
    return stop;
}

// The walk of one token's bytes from (q, d) under the grammar's table, as grammar_apply_kernel and grammar_advance_kernel make it:
// the token's own pushes go to the thread's column of `win` (slot-major, `stride` columns), pops below them read stack_at(level).
// False: the walk died (a token of no bytes included); q, d and own are then meaningless.
template <class StackAt>
__device__ __forceinline__ bool lane_grammar_walk(const GrammarView* view, uint32_t S, const uint8_t* __restrict__ flags, int tok, uint32_t& q,
                                                  int& d, int& own, uint16_t* win, int stride, StackAt stack_at)
{
    const uint32_t* __restrict__ action = view->action;
    const uint8_t* __restrict__ bytes = view->tok_bytes;
    const uint32_t lo = view->tok_off[tok], hi = view->tok_off[tok + 1];
    bool alive = hi > lo;
    for (uint32_t i = lo; i < hi && alive; ++i) {
        const uint32_t b = bytes[i];
        for (int steps = 0;; ++steps) {
            if (steps >= kGrammarMaxByteSteps) {  // (never with a table from the compiler; the host's walk has the same bound)
                alive = false;
                break;
            }
            const uint32_t a = action[q * 256u + b];
            const uint32_t kind = a >> 30;
            if (kind == 1) {
                q = a & 0xFFFu;
                break;
            }
            if (kind == 2) {
                if (d >= kGrammarMaxDepth || own >= kGrammarTokenPushes) {
                    alive = false;
                    break;
                }
                win[own * stride] = (uint16_t)((a >> 12) & 0xFFFu);
                ++own;
                ++d;
                q = a & 0xFFFu;
                continue;
            }
            if (!(flags[q] & kGrammarAccepting) || d <= 0) {
                alive = false;
                break;
            }
            --d;
            if (own > 0) {
                --own;
                q = win[own * stride];
            } else {
                q = stack_at(d);
            }
            if (q >= S) {  // (an action table that names no state: never from the compiler)
                alive = false;
                break;
            }
        }
    }
    return alive;
}

// blockIdx.y + first_lane is the lane; one thread per logit.  Every early return is uniform per workgroup.  A grammar lane stages
// its stack in LDS once per workgroup, with the verdict on it (every level accepting: what a stop id needs), and keeps each
// token's own pushes in the thread's column of s_win.  Allowed logits are not rewritten, so they keep their bits.
__global__ __launch_bounds__(kApplyThreads) void lane_automaton_apply_kernel(float* __restrict__ logits, int64_t ld, int vocab, int first_lane,
                                                                             const LaneAutomatonTable* __restrict__ table,
                                                                             const int32_t* __restrict__ live)
{
    __shared__ uint16_t s_stack[kGrammarMaxDepth];
    __shared__ uint16_t s_win[kGrammarTokenPushes * kApplyThreads];
    __shared__ int s_verdict;  // bit 0: a level below the state is not accepting; bit 1: a stack word names no state
    const int l = first_lane + blockIdx.y, tid = threadIdx.x;
    if (l >= kLaneAutomatonSlots || !live[l]) return;
    const LaneAutomatonSlot* slot = table->slot + l;
    const int kind = slot->kind;
    const int v = blockIdx.x * kApplyThreads + tid;
    float* row = logits + (int64_t)l * ld;
    if (kind == kLaneKindPattern) {
        const ConstraintView* view = &slot->cview;
        const ConstraintRow rs = slot->crow;
        if (rs.done) return;
        const uint32_t q = rs.state;
        if (q >= (uint32_t)view->states) return;  // (no such state: advance flags it; nothing is read out of range)
        if (v >= vocab) return;
        bool allowed;
        if (lane_is_stop(view->stops, view->n_stop, (uint32_t)v)) allowed = (view->flags[q] & kFlagAccepting) != 0;
        else allowed = v < view->vocab && ((view->mask[(size_t)q * view->words + (v >> 6)] >> (v & 63)) & 1ull) != 0;
        if (!allowed) row[v] = -INFINITY;
        return;
    }
    if (kind != kLaneKindGrammar) return;
    const GrammarView* view = &slot->gview;
    const GrammarRow* rs = &slot->grow;
    if (rs->done) return;
    const uint32_t S = (uint32_t)view->states;
    const uint32_t q0 = rs->state;
    const int d0 = rs->depth;
    if (q0 >= S || d0 < 0 || d0 > kGrammarMaxDepth) return;  // no configuration: advance flags it
    const uint8_t* __restrict__ flags = view->flags;
    if (tid == 0) s_verdict = 0;
    __syncthreads();
    if (tid < kGrammarMaxDepth) {
        const uint16_t s = tid < d0 ? rs->stack[tid] : (uint16_t)0;
        s_stack[tid] = s;
        if (tid < d0) {
            if (s >= S) atomicOr(&s_verdict, 2);
            else if (!(flags[s] & kGrammarAccepting)) atomicOr(&s_verdict, 1);
        }
    }
    __syncthreads();
    const int verdict = s_verdict;
    if (verdict & 2) return;
    if (v >= vocab) return;  // (no barrier follows)
    bool allowed;
    if (lane_is_stop(view->stops, view->n_stop, (uint32_t)v)) {
        allowed = verdict == 0 && (flags[q0] & kGrammarAccepting) != 0;
    } else if (v >= view->vocab) {
        allowed = false;
    } else {
        uint32_t q = q0;
        int d = d0, own = 0;
        allowed = lane_grammar_walk(view, S, flags, v, q, d, own, s_win + tid, kApplyThreads, [&](int level) { return (uint32_t)s_stack[level]; });
    }
    if (!allowed) row[v] = -INFINITY;
}

// constraint_advance_kernel on the lane's own view and row (the row is not done).
__device__ __forceinline__ void lane_pattern_advance(const ConstraintView* view, ConstraintRow* row, int32_t tok)
{
    ConstraintRow rs = *row;
    const uint32_t S = (uint32_t)view->states;
    uint32_t q = rs.state;
    bool dead = q >= S;
    if (!dead && tok >= 0 && lane_is_stop(view->stops, view->n_stop, (uint32_t)tok)) {
        if (view->flags[q] & kFlagAccepting) {
            rs.done = 1;
            *row = rs;
            return;
        }
        dead = true;  // a stop id outside an accepting state is masked
    }
    if (!dead && (tok < 0 || tok >= view->vocab)) dead = true;
    if (!dead) {
        const uint32_t lo = view->tok_off[tok], hi = view->tok_off[tok + 1];
        dead = hi <= lo;
        for (uint32_t i = lo; i < hi && !dead; ++i) {
            q = view->trans[(size_t)q * 256 + view->tok_bytes[i]];
            dead = q >= S;
        }
    }
    if (dead) {
        rs.violated = 1;
        rs.done = 1;
    } else {
        rs.state = q;
        if (view->flags[q] & kFlagClosed) rs.done = 1;
    }
    *row = rs;
}

// grammar_advance_kernel on the lane's own view and row (the row is not done): only a walk that lived is written back, the stack
// words from the lowest depth the walk reached up to the new depth and nothing above.
__device__ __forceinline__ void lane_grammar_advance(const GrammarView* view, GrammarRow* rs, int32_t tok, uint16_t* win)
{
    uint32_t q = rs->state;
    int d = rs->depth;
    const uint32_t S = (uint32_t)view->states;
    const uint8_t* __restrict__ flags = view->flags;
    bool dead = q >= S || d < 0 || d > kGrammarMaxDepth;
    bool accepted = !dead && (flags[q] & kGrammarAccepting) != 0;
    if (!dead)
        for (int i = 0; i < d; ++i) {
            const uint32_t s = rs->stack[i];
            if (s >= S) {
                dead = true;
                break;
            }
            accepted = accepted && (flags[s] & kGrammarAccepting) != 0;
        }
    if (!dead && tok >= 0 && lane_is_stop(view->stops, view->n_stop, (uint32_t)tok)) {
        if (accepted) {
            rs->done = 1;
            return;
        }
        dead = true;  // a stop id outside an accepted configuration is masked
    }
    if (!dead && (tok < 0 || tok >= view->vocab)) dead = true;
    int own = 0;
    if (!dead) dead = !lane_grammar_walk(view, S, flags, tok, q, d, own, win, kAdvanceThreads, [&](int level) { return (uint32_t)rs->stack[level]; });
    if (dead) {
        rs->violated = 1;
        rs->done = 1;
        return;
    }
    for (int i = 0; i < own; ++i) rs->stack[d - own + i] = win[i * kAdvanceThreads];  // (d <= kGrammarMaxDepth: the walk checked every push)
    rs->state = q;
    rs->depth = d;
    bool closed = (flags[q] & kGrammarNoOut) != 0;
    for (int i = 0; i < d && closed; ++i) closed = (flags[rs->stack[i]] & kGrammarNoOut) != 0;
    if (closed) rs->done = 1;
}

// One thread per lane of [first_lane, first_lane + lanes), behind the pick's finalize.  live / count are the arrays of an
// LlmLaneState or an LlmWideState: the kernel serves both layouts.
__global__ __launch_bounds__(kAdvanceThreads) void lane_automaton_advance_kernel(LaneAutomatonTable* __restrict__ table, int first_lane, int lanes,
                                                                                 int32_t* __restrict__ live, const int32_t* __restrict__ count,
                                                                                 const int32_t* __restrict__ history, int hist_stride)
{
    __shared__ uint16_t s_win[kGrammarTokenPushes * kAdvanceThreads];
    const int tid = threadIdx.x, l = first_lane + tid;
    if (tid >= lanes || l >= kLaneAutomatonSlots) return;
    LaneAutomatonSlot* slot = table->slot + l;
    const int cnt = count[l];
    if (cnt <= slot->walked) {  // the pick skipped the lane: it was not live
        table->fresh[l] = 0;
        return;
    }
    const int at = cnt - 1;
    const int32_t tok = at >= 0 && at < hist_stride ? history[(int64_t)l * hist_stride + at] : -1;
    slot->walked = cnt;
    table->fresh[l] = 1;
    table->picked[l] = tok;
    const int kind = slot->kind;
    int done = 0;
    if (kind == kLaneKindPattern) {
        if (slot->crow.done) return;
        lane_pattern_advance(&slot->cview, &slot->crow, tok);
        done = slot->crow.done;
    } else if (kind == kLaneKindGrammar) {
        if (slot->grow.done) return;
        lane_grammar_advance(&slot->gview, &slot->grow, tok, s_win + tid);
        done = slot->grow.done;
    }
    if (done) live[l] = 0;  // accepted stop id, closed, or a dead walk: nothing more is fed (the token stays in the history)
}

}  // namespace

hipError_t launch_lane_automaton_apply(float* logits, int64_t ld, int vocab, int lanes, int first_lane, const LaneAutomatonTable* table,
                                       const int32_t* live, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (first_lane < 0 || first_lane + lanes > kLaneAutomatonSlots || vocab < 1 || ld < vocab || !logits || !table || !live) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_automaton_apply_kernel, dim3((unsigned)((vocab + kApplyThreads - 1) / kApplyThreads), (unsigned)lanes), dim3(kApplyThreads),
                       0, stream, logits, ld, vocab, first_lane, table, live);
    return hipGetLastError();
}

hipError_t launch_lane_automaton_advance(LaneAutomatonTable* table, int lanes, int first_lane, int32_t* live, const int32_t* count,
                                         const int32_t* history, int hist_stride, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (first_lane < 0 || first_lane + lanes > kLaneAutomatonSlots || hist_stride < 1 || !table || !live || !count || !history) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_automaton_advance_kernel, dim3(1), dim3(kAdvanceThreads), 0, stream, table, first_lane, lanes, live, count, history,
                       hist_stride);
    return hipGetLastError();
}

hipError_t launch_lane_automaton_pick(const float* logits, int64_t ld, int vocab, int lanes, int first_lane, unsigned long long* best_scratch,
                                      LaneStateRef state, int32_t* history, int hist_stride, int capacity, int advance,
                                      LaneAutomatonTable* table, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;  // (the range, vocab and hist_stride are launch_lane_pick's refusals)
    const hipError_t e = launch_lane_pick(logits, ld, vocab, lanes, first_lane, best_scratch, state, history, hist_stride, capacity, advance, stream);
    if (e != hipSuccess) return e;
    return launch_lane_automaton_advance(table, lanes, first_lane, state.live, state.count, history, hist_stride, stream);
}

}  // namespace kjarni
