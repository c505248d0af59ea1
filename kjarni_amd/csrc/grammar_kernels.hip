// Grammar-constrained decoding kernels for gfx950 (grammar_kernels.h) and the device object that owns a grammar's tables.
#include "grammar_kernels.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "ffi_common.h"
#include "host_util.h"

namespace kjarni {

namespace {

constexpr int kApplyThreads = 256, kAdvanceThreads = 64;

__device__ __forceinline__ bool grammar_is_stop(const GrammarView* view, uint32_t v)
{
    bool stop = false;
    const int n = view->n_stop;
    for (int i = 0; i < n && i < kConstraintMaxStops; ++i) stop |= view->stops[i] == v;
    return stop;
}

// blockIdx.y is the row; one thread per token.  The row's stack is staged in LDS once per workgroup, with the verdict on it
// (every level accepting: what a stop id needs).  A thread keeps its token's own pushes in its column of s_win (slot-major, so
// the lanes of a wave touch consecutive halfwords); pops below them read the staged stack and never write it.  Allowed logits are
// not rewritten, so they keep their bits.
__global__ __launch_bounds__(kApplyThreads) void grammar_apply_kernel(float* __restrict__ logits, int64_t ld, const GrammarView* __restrict__ view,
                                                                      const GrammarRow* __restrict__ row_state)
{
    __shared__ uint16_t s_stack[kGrammarMaxDepth];
    __shared__ uint16_t s_win[kGrammarTokenPushes * kApplyThreads];
    __shared__ int s_verdict;  // bit 0: a level below the state is not accepting; bit 1: a stack word names no state
    const int r = blockIdx.y, tid = threadIdx.x;
    const GrammarRow* rs = row_state + r;
    if (rs->done) return;  // (uniform per workgroup, as the two returns below)
    const uint32_t S = (uint32_t)view->states;
    const uint32_t q0 = rs->state;
    const int d0 = rs->depth;
    if (q0 >= S || d0 < 0 || d0 > kGrammarMaxDepth) return;  // no configuration: advance flags it; nothing is read out of range
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
    const int v = blockIdx.x * kApplyThreads + tid;
    if (v >= view->vocab) return;  // (no barrier follows)
    bool allowed;
    if (grammar_is_stop(view, (uint32_t)v)) {
        allowed = verdict == 0 && (flags[q0] & kGrammarAccepting) != 0;
    } else {
        const uint32_t* __restrict__ action = view->action;
        const uint8_t* __restrict__ bytes = view->tok_bytes;
        const uint32_t lo = view->tok_off[v], hi = view->tok_off[v + 1];
        uint32_t q = q0;
        int d = d0, own = 0;
        allowed = hi > lo;
        for (uint32_t i = lo; i < hi && allowed; ++i) {
            const uint32_t b = bytes[i];
            for (int steps = 0;; ++steps) {
                if (steps >= kGrammarMaxByteSteps) {  // (never with a table from the compiler; the host's walk has the same bound)
                    allowed = false;
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
                        allowed = false;
                        break;
                    }
                    s_win[own * kApplyThreads + tid] = (uint16_t)((a >> 12) & 0xFFFu);
                    ++own;
                    ++d;
                    q = a & 0xFFFu;
                    continue;
                }
                if (!(flags[q] & kGrammarAccepting) || d <= 0) {
                    allowed = false;
                    break;
                }
                --d;
                if (own > 0) {
                    --own;
                    q = s_win[own * kApplyThreads + tid];
                } else {
                    q = s_stack[d];
                }
                if (q >= S) {  // (an action table that names no state: never from the compiler)
                    allowed = false;
                    break;
                }
            }
        }
    }
    if (!allowed) logits[(int64_t)r * ld + v] = -INFINITY;
}

__device__ __forceinline__ void grammar_log(uint32_t* state_log, int32_t* depth_log, const int* count, int log_cap, uint32_t state, int32_t depth)
{
    if (!state_log) return;
    const int at = *count - 1;
    if (at >= 0 && at < log_cap) {
        state_log[at] = state;
        depth_log[at] = depth;
    }
}

// One thread per row.  A stop id in an accepted configuration keeps the configuration and sets done; any other token walks its
// bytes as apply does, its own pushes in the thread's column of s_win, and only a walk that lived is written back: the stack words
// from the lowest depth the walk reached up to the new depth, nothing above.  Done when every level is then no_out.  A token
// apply would have masked sets violated and done and moves nothing.
__global__ __launch_bounds__(kAdvanceThreads) void grammar_advance_kernel(const int32_t* __restrict__ picked, int rows, const GrammarView* __restrict__ view,
                                                                          GrammarRow* __restrict__ row_state, uint32_t* __restrict__ state_log,
                                                                          int32_t* __restrict__ depth_log, const int* __restrict__ count, int log_cap)
{
    __shared__ uint16_t s_win[kGrammarTokenPushes * kAdvanceThreads];
    const int tid = threadIdx.x;
    const int r = blockIdx.x * kAdvanceThreads + tid;
    if (r >= rows) return;
    GrammarRow* rs = row_state + r;
    uint32_t q = rs->state;
    int d = rs->depth;
    if (rs->done) {
        grammar_log(state_log, depth_log, count, log_cap, q, d);
        return;
    }
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
    const int32_t tok = picked[r];
    if (!dead && tok >= 0 && grammar_is_stop(view, (uint32_t)tok)) {
        if (accepted) {
            rs->done = 1;
            grammar_log(state_log, depth_log, count, log_cap, q, d);
            return;
        }
        dead = true;  // a stop id outside an accepted configuration is masked
    }
    if (!dead && (tok < 0 || tok >= view->vocab)) dead = true;
    int own = 0;
    if (!dead) {
        const uint32_t* __restrict__ action = view->action;
        const uint32_t lo = view->tok_off[tok], hi = view->tok_off[tok + 1];
        dead = hi <= lo;
        for (uint32_t i = lo; i < hi && !dead; ++i) {
            const uint32_t b = view->tok_bytes[i];
            for (int steps = 0;; ++steps) {
                if (steps >= kGrammarMaxByteSteps) {
                    dead = true;
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
                        dead = true;
                        break;
                    }
                    s_win[own * kAdvanceThreads + tid] = (uint16_t)((a >> 12) & 0xFFFu);
                    ++own;
                    ++d;
                    q = a & 0xFFFu;
                    continue;
                }
                if (!(flags[q] & kGrammarAccepting) || d <= 0) {
                    dead = true;
                    break;
                }
                --d;
                if (own > 0) {
                    --own;
                    q = s_win[own * kAdvanceThreads + tid];
                } else {
                    q = rs->stack[d];  // (checked above: a state of the table)
                }
                if (q >= S) {
                    dead = true;
                    break;
                }
            }
        }
    }
    if (dead) {
        rs->violated = 1;
        rs->done = 1;
        grammar_log(state_log, depth_log, count, log_cap, rs->state, rs->depth);
        return;
    }
    for (int i = 0; i < own; ++i) rs->stack[d - own + i] = s_win[i * kAdvanceThreads + tid];  // (d <= kGrammarMaxDepth: the walk checked every push)
    rs->state = q;
    rs->depth = d;
    bool closed = (flags[q] & kGrammarNoOut) != 0;
    for (int i = 0; i < d && closed; ++i) closed = (flags[rs->stack[i]] & kGrammarNoOut) != 0;
    if (closed) rs->done = 1;
    grammar_log(state_log, depth_log, count, log_cap, q, d);
}

}  // namespace

hipError_t launch_grammar_apply(float* logits, int64_t ld, int rows, int vocab, const GrammarView* view, const GrammarRow* row_state, hipStream_t stream)
{
    if (rows < 1 || rows > 65535 || vocab < 1 || ld < vocab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grammar_apply_kernel, dim3((unsigned)((vocab + kApplyThreads - 1) / kApplyThreads), (unsigned)rows), dim3(kApplyThreads), 0, stream,
                       logits, ld, view, row_state);
    return hipGetLastError();
}

hipError_t launch_grammar_advance(const int32_t* picked, int rows, const GrammarView* view, GrammarRow* row_state, uint32_t* state_log,
                                  int32_t* depth_log, const int* count, int log_cap, hipStream_t stream)
{
    if (rows < 1 || (state_log == nullptr) != (depth_log == nullptr) || (state_log && (rows != 1 || !count || log_cap < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grammar_advance_kernel, dim3((unsigned)((rows + kAdvanceThreads - 1) / kAdvanceThreads)), dim3(kAdvanceThreads), 0, stream, picked,
                       rows, view, row_state, state_log, depth_log, count, log_cap);
    return hipGetLastError();
}

// ---- the device object ---------------------------------------------------------------------------------------------------------

DeviceGrammar::DeviceGrammar(int device, Grammar grammar, TokenTable table) : device_(device), grammar_(std::move(grammar)), table_(std::move(table))
{
    const int S = grammar_.states(), V = table_.vocab();
    if (S < 1 || S > kGrammarMaxStates || grammar_.action.size() != (size_t)S * 256) throw InvalidConfig("grammar: malformed automaton");
    for (size_t i = 0; i < grammar_.action.size(); ++i) {
        const uint32_t a = grammar_.action[i], kind = a >> 30;
        if (kind > 2 || (kind && (a & 0xFFFu) >= (uint32_t)S) || (kind == 2 && ((a >> 12) & 0xFFFu) >= (uint32_t)S))
            throw InvalidConfig("grammar: the action table names a state that does not exist");
    }
    if (V < 1) throw InvalidConfig("grammar: the token table is empty");
    if (table_.off[0] != 0 || table_.off[(size_t)V] != table_.bytes.size())
        throw InvalidConfig("grammar: tok_off must start at 0 and end at the number of token bytes");
    for (int t = 0; t < V; ++t)
        if (table_.off[(size_t)t + 1] < table_.off[(size_t)t]) throw InvalidConfig("grammar: tok_off decreases at token " + std::to_string(t));
    if (grammar_.rule_of.size() != (size_t)S) throw InvalidConfig("grammar: malformed automaton");
    if (visible_device_count() <= device || device < 0) throw GpuUnavailable("no usable HIP device " + std::to_string(device));
    analyse();
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t action_b = pad((size_t)S * 1024), flags_b = pad((size_t)S), off_b = pad(((size_t)V + 1) * 4), bytes_b = pad(table_.bytes.size() + 1);
    hip_check(hipMalloc(&block_, action_b + flags_b + off_b + bytes_b), "hipMalloc(grammar tables)");
    uint8_t* at = static_cast<uint8_t*>(block_);
    action_ = reinterpret_cast<uint32_t*>(at);
    flags_ = at + action_b;
    off_ = reinterpret_cast<uint32_t*>(at + action_b + flags_b);
    bytes_ = at + action_b + flags_b + off_b;
    try {
        hip_check(hipMemcpy(action_, grammar_.action.data(), (size_t)S * 1024, hipMemcpyHostToDevice), "H2D grammar table");
        hip_check(hipMemcpy(flags_, grammar_.flags.data(), (size_t)S, hipMemcpyHostToDevice), "H2D grammar flags");
        hip_check(hipMemcpy(off_, table_.off.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice), "H2D token offsets");
        if (!table_.bytes.empty()) hip_check(hipMemcpy(bytes_, table_.bytes.data(), table_.bytes.size(), hipMemcpyHostToDevice), "H2D token bytes");
    } catch (...) {
        (void)hipFree(block_);
        throw;
    }
}

DeviceGrammar::~DeviceGrammar()
{
    (void)hipSetDevice(device_);
    if (block_) (void)hipFree(block_);
}

bool DeviceGrammar::explore(uint32_t q0, uint32_t t, std::vector<uint16_t>* ends) const
{
    const uint8_t* bytes = table_.token(t);
    const size_t n = table_.length(t);
    if (n == 0) return false;
    const std::vector<uint32_t>& action = grammar_.action;
    const std::vector<uint8_t>& flags = grammar_.flags;
    // depth-first over (byte index, state, own pushes); a branch with no own pushes is visited once per (index, state)
    struct Branch {
        size_t i;
        uint32_t q;
        std::vector<uint16_t> own;
    };
    thread_local std::vector<Branch> todo;  // (kept across calls: the analysis walks every token from every reachable state)
    thread_local std::vector<std::pair<size_t, uint32_t>> seen;
    todo.clear();
    seen.clear();
    todo.push_back({0, q0, {}});
    bool alive = false;
    while (!todo.empty()) {
        Branch b = std::move(todo.back());
        todo.pop_back();
        bool dead = false;
        while (b.i < n && !dead) {
            for (int steps = 0;; ++steps) {
                if (steps >= kGrammarMaxByteSteps) {
                    dead = true;
                    break;
                }
                const uint32_t a = action[(size_t)b.q * 256 + bytes[b.i]];
                if ((a >> 30) == 1) {
                    b.q = a & 0xFFFu;
                    break;
                }
                if ((a >> 30) == 2) {
                    if (b.own.size() >= (size_t)kGrammarTokenPushes) {
                        dead = true;
                        break;
                    }
                    b.own.push_back((uint16_t)((a >> 12) & 0xFFFu));
                    b.q = a & 0xFFFu;
                    continue;
                }
                if (!(flags[b.q] & kGrammarAccepting)) {
                    dead = true;
                    break;
                }
                if (!b.own.empty()) {
                    b.q = b.own.back();
                    b.own.pop_back();
                    continue;
                }
                for (uint16_t r : returns_[grammar_.rule_of[b.q]]) {  // below the token's own pushes: wherever the rule was called from
                    const std::pair<size_t, uint32_t> key(b.i, r);
                    if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
                    seen.push_back(key);
                    todo.push_back({b.i, r, {}});
                }
                dead = true;  // (this branch goes on in those)
                break;
            }
            if (!dead) ++b.i;
        }
        if (dead) continue;
        alive = true;
        if (!ends) return true;
        ends->push_back((uint16_t)b.q);
    }
    return alive;
}

void DeviceGrammar::analyse()
{
    const size_t S = (size_t)grammar_.states(), V = (size_t)vocab();
    size_t rules = 0;
    for (uint16_t r : grammar_.rule_of) rules = std::max(rules, (size_t)r + 1);
    returns_.assign(rules, {});
    for (size_t i = 0; i < grammar_.action.size(); ++i) {
        const uint32_t a = grammar_.action[i];
        if ((a >> 30) != 2) continue;
        std::vector<uint16_t>& list = returns_[grammar_.rule_of[a & 0xFFFu]];
        const uint16_t ret = (uint16_t)((a >> 12) & 0xFFFu);
        if (std::find(list.begin(), list.end(), ret) == list.end()) list.push_back(ret);
    }
    // the tokens by their first byte: a state that neither moves, calls nor can end on that byte skips them all
    std::vector<std::vector<uint32_t>> by_first(256);
    for (size_t t = 0; t < V; ++t)
        if (table_.length((uint32_t)t) > 0) by_first[table_.token((uint32_t)t)[0]].push_back((uint32_t)t);
    reachable_.assign(S, 0);
    offered_.assign(S, 0);
    std::vector<uint32_t> todo = {0};
    std::vector<uint16_t> ends;
    reachable_[0] = 1;
    while (!todo.empty()) {
        const uint32_t q = todo.back();
        todo.pop_back();
        for (int b = 0; b < 256; ++b) {
            if (by_first[(size_t)b].empty()) continue;
            if ((grammar_.action[(size_t)q * 256 + (size_t)b] >> 30) == 0 && !(grammar_.flags[q] & kGrammarAccepting)) continue;
            for (uint32_t t : by_first[(size_t)b]) {
                ends.clear();
                if (!explore(q, t, &ends)) continue;
                ++offered_[q];
                for (uint16_t e : ends)
                    if (!reachable_[e]) {
                        reachable_[e] = 1;
                        todo.push_back(e);
                    }
            }
        }
    }
}

void DeviceGrammar::check_states(const std::vector<uint32_t>& stops) const
{
    if (stops.size() > (size_t)kConstraintMaxStops)
        throw InvalidConfig("a constrained call takes at most " + std::to_string(kConstraintMaxStops) + " stop ids, got " + std::to_string(stops.size()));
    std::vector<uint32_t> distinct;
    for (uint32_t s : stops)
        if (std::find(distinct.begin(), distinct.end(), s) == distinct.end()) distinct.push_back(s);
    for (uint32_t q = 0; q < (uint32_t)grammar_.states(); ++q) {
        if (!reachable_[q]) continue;
        uint32_t free_tokens = offered_[q];
        for (uint32_t s : distinct)
            if (s < (uint32_t)vocab() && explore(q, s, nullptr)) --free_tokens;  // (a stop id is governed by the accepted rule alone)
        if (free_tokens > 0) continue;
        const uint8_t f = grammar_.flags[q];
        const std::string where = "grammar: state " + std::to_string(q) + " (rule '" + grammar_.rules[grammar_.rule_of[q]] + "')";
        if (!(f & kGrammarAccepting))
            throw InvalidConfig(where + " allows no token of this vocabulary (the rule can neither go on nor end there)");
        if (grammar_.rule_of[q] == 0 && !(f & kGrammarNoOut) && stops.empty())
            throw InvalidConfig(where + " allows no token of this vocabulary and the call has no stop id to end on");
    }
}

GrammarView DeviceGrammar::view(const std::vector<uint32_t>& stops) const
{
    if (stops.size() > (size_t)kConstraintMaxStops)
        throw InvalidConfig("a constrained call takes at most " + std::to_string(kConstraintMaxStops) + " stop ids, got " + std::to_string(stops.size()));
    GrammarView v = {};
    v.action = action_;
    v.flags = flags_;
    v.tok_off = off_;
    v.tok_bytes = bytes_;
    v.states = grammar_.states();
    v.vocab = vocab();
    v.n_stop = (int32_t)stops.size();
    for (size_t i = 0; i < stops.size(); ++i) v.stops[i] = stops[i];
    return v;
}

}  // namespace kjarni
