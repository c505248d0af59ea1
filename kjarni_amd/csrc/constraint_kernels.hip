// Constrained decoding kernels for gfx950 (constraint_kernels.h) and the device object that owns a constraint's tables.
#include "constraint_kernels.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "ffi_common.h"
#include "host_util.h"

namespace kjarni {

namespace {

constexpr uint8_t kFlagAccepting = 1, kFlagClosed = 2;

// One thread per (state, token): blockIdx.y is the state, a wave covers the 64 consecutive tokens of one mask word.  The wave's
// ballot (64 bits on gfx950) is the word; lane 0 stores it and adds its population count to the state's counter.  The table
// (states x 512 bytes) is read by every wave of a row and stays in L2; the token bytes are read once per state.
__global__ __launch_bounds__(256) void constraint_mask_kernel(const uint16_t* __restrict__ trans, int states, const uint32_t* __restrict__ tok_off,
                                                              const uint8_t* __restrict__ tok_bytes, int vocab, int words,
                                                              unsigned long long* __restrict__ mask, uint32_t* __restrict__ count)
{
    const int lane = threadIdx.x & 63;
    const int word = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int q0 = blockIdx.y;
    if (word >= words) return;  // (uniform per wave; no barrier follows)
    const int t = word * 64 + lane;
    bool ok = false;
    if (t < vocab) {
        const uint32_t lo = tok_off[t], hi = tok_off[t + 1];
        uint32_t q = (uint32_t)q0;
        ok = hi > lo;
        for (uint32_t i = lo; i < hi; ++i) {
            q = trans[(size_t)q * 256 + tok_bytes[i]];
            if (q >= (uint32_t)states) {  // kConstraintDead (or a table that names no state)
                ok = false;
                break;
            }
        }
    }
    const unsigned long long bits = __ballot(ok);
    if (lane == 0) {
        mask[(size_t)q0 * words + word] = bits;
        if (bits) atomicAdd(count + q0, (uint32_t)__popcll(bits));
    }
}

__device__ __forceinline__ bool constraint_is_stop(const ConstraintView* view, uint32_t v)
{
    bool stop = false;
    const int n = view->n_stop;
    for (int i = 0; i < n && i < kConstraintMaxStops; ++i) stop |= view->stops[i] == v;
    return stop;
}

// blockIdx.y is the row; one thread per logit.  Allowed logits are not rewritten, so they keep their bits.
__global__ __launch_bounds__(256) void constraint_apply_kernel(float* __restrict__ logits, int64_t ld, int vocab,
                                                               const ConstraintView* __restrict__ view,
                                                               const ConstraintRow* __restrict__ row_state)
{
    const int r = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= vocab) return;
    const ConstraintRow rs = row_state[r];
    if (rs.done) return;
    const uint32_t q = rs.state;
    if (q >= (uint32_t)view->states) return;  // (no such state: advance would have flagged it; nothing is read out of range)
    bool allowed;
    if (constraint_is_stop(view, (uint32_t)v)) allowed = (view->flags[q] & kFlagAccepting) != 0;
    else allowed = v < view->vocab && ((view->mask[(size_t)q * view->words + (v >> 6)] >> (v & 63)) & 1ull) != 0;
    if (!allowed) logits[(int64_t)r * ld + v] = -INFINITY;
}

// One thread per row.  A stop id in an accepting state keeps the state and sets done; any other token walks its bytes (done
// when the new state is closed); a token the mask would not have allowed sets violated and freezes the row.  state_log (rows == 1,
// may be null): the row's state after this step goes to state_log[*count - 1], next to the pick launch_argmax recorded at that index.
__device__ __forceinline__ void constraint_log(uint32_t* state_log, const int* count, int log_cap, uint32_t state)
{
    if (!state_log) return;
    const int at = *count - 1;
    if (at >= 0 && at < log_cap) state_log[at] = state;
}

__global__ void constraint_advance_kernel(const int32_t* __restrict__ picked, int rows, const ConstraintView* __restrict__ view,
                                          ConstraintRow* __restrict__ row_state, uint32_t* __restrict__ state_log,
                                          const int* __restrict__ count, int log_cap)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    ConstraintRow rs = row_state[r];
    if (rs.done) {
        constraint_log(state_log, count, log_cap, rs.state);
        return;
    }
    const int32_t tok = picked[r];
    const uint32_t S = (uint32_t)view->states;
    uint32_t q = rs.state;
    bool dead = q >= S;
    if (!dead && tok >= 0 && constraint_is_stop(view, (uint32_t)tok)) {
        if (view->flags[q] & kFlagAccepting) {
            rs.done = 1;
            row_state[r] = rs;
            constraint_log(state_log, count, log_cap, rs.state);
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
    row_state[r] = rs;
    constraint_log(state_log, count, log_cap, rs.state);
}

}  // namespace

hipError_t launch_constraint_mask(const uint16_t* trans, int states, const uint32_t* tok_off, const uint8_t* tok_bytes, int vocab,
                                  unsigned long long* mask, uint32_t* count, hipStream_t stream)
{
    const int words = (vocab + 63) / 64;
    if (states < 1 || states > kConstraintMaxStates || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(constraint_mask_kernel, dim3((unsigned)((words + 3) / 4), (unsigned)states), dim3(256), 0, stream, trans, states, tok_off,
                       tok_bytes, vocab, words, mask, count);
    return hipGetLastError();
}

hipError_t launch_constraint_apply(float* logits, int64_t ld, int rows, int vocab, const ConstraintView* view, const ConstraintRow* row_state,
                                   hipStream_t stream)
{
    if (rows < 1 || vocab < 1 || ld < vocab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(constraint_apply_kernel, dim3((unsigned)((vocab + 255) / 256), (unsigned)rows), dim3(256), 0, stream, logits, ld, vocab, view,
                       row_state);
    return hipGetLastError();
}

hipError_t launch_constraint_advance(const int32_t* picked, int rows, const ConstraintView* view, ConstraintRow* row_state, uint32_t* state_log,
                                     const int* count, int log_cap, hipStream_t stream)
{
    if (rows < 1 || (state_log && (rows != 1 || !count || log_cap < 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(constraint_advance_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, stream, picked, rows, view, row_state, state_log,
                       count, log_cap);
    return hipGetLastError();
}

// ---- the device object ---------------------------------------------------------------------------------------------------------

DeviceConstraint::DeviceConstraint(int device, ConstraintDfa dfa, TokenTable table) : device_(device), dfa_(std::move(dfa)), table_(std::move(table))
{
    const int S = dfa_.states(), V = table_.vocab();
    if (S < 1 || S > kConstraintMaxStates || dfa_.trans.size() != (size_t)S * 256) throw InvalidConfig("constraint: malformed automaton");
    if (V < 1) throw InvalidConfig("constraint: the token table is empty");
    if (table_.off[0] != 0 || table_.off[(size_t)V] != table_.bytes.size())
        throw InvalidConfig("constraint: tok_off must start at 0 and end at the number of token bytes");
    for (int t = 0; t < V; ++t)
        if (table_.off[(size_t)t + 1] < table_.off[(size_t)t])
            throw InvalidConfig("constraint: tok_off decreases at token " + std::to_string(t));
    const size_t W = (size_t)words(), mask_bytes = (size_t)S * W * 8;
    if (mask_bytes > kConstraintMaxMaskBytes)
        throw InvalidConfig("constraint: the token mask of " + std::to_string(S) + " states x " + std::to_string(V) + " tokens needs " +
                            std::to_string(mask_bytes) + " bytes, the limit is " + std::to_string(kConstraintMaxMaskBytes));
    if (visible_device_count() <= device || device < 0) throw GpuUnavailable("no usable HIP device " + std::to_string(device));
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t trans_b = pad((size_t)S * 512), flags_b = pad((size_t)S), off_b = pad(((size_t)V + 1) * 4),
                 bytes_b = pad(table_.bytes.size() + 1), count_b = pad((size_t)S * 4);
    hip_check(hipMalloc(&block_, trans_b + flags_b + off_b + bytes_b + count_b), "hipMalloc(constraint tables)");
    uint8_t* at = static_cast<uint8_t*>(block_);
    trans_ = reinterpret_cast<uint16_t*>(at);
    flags_ = at + trans_b;
    off_ = reinterpret_cast<uint32_t*>(at + trans_b + flags_b);
    bytes_ = at + trans_b + flags_b + off_b;
    count_ = reinterpret_cast<uint32_t*>(at + trans_b + flags_b + off_b + bytes_b);
    try {
        hip_check(hipMalloc((void**)&mask_, mask_bytes), "hipMalloc(constraint mask)");
        std::vector<uint8_t> flags((size_t)S);
        for (int q = 0; q < S; ++q) flags[(size_t)q] = (uint8_t)((dfa_.accepting[(size_t)q] ? kFlagAccepting : 0) | (dfa_.closed[(size_t)q] ? kFlagClosed : 0));
        hip_check(hipMemcpy(trans_, dfa_.trans.data(), (size_t)S * 512, hipMemcpyHostToDevice), "H2D constraint table");
        hip_check(hipMemcpy(flags_, flags.data(), (size_t)S, hipMemcpyHostToDevice), "H2D constraint flags");
        hip_check(hipMemcpy(off_, table_.off.data(), ((size_t)V + 1) * 4, hipMemcpyHostToDevice), "H2D token offsets");
        if (!table_.bytes.empty()) hip_check(hipMemcpy(bytes_, table_.bytes.data(), table_.bytes.size(), hipMemcpyHostToDevice), "H2D token bytes");
        hip_check(hipMemset(count_, 0, (size_t)S * 4), "memset counts");
        hip_check(launch_constraint_mask(trans_, S, off_, bytes_, V, mask_, count_, nullptr), "constraint mask");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        counts_.resize((size_t)S);
        hip_check(hipMemcpy(counts_.data(), count_, (size_t)S * 4, hipMemcpyDeviceToHost), "D2H counts");
        // the states a run can be in: the start state and whatever the allowed tokens lead to (a state in the middle of a
        // multi-byte character is one no run reaches when every token holds whole characters)
        reachable_.assign((size_t)S, 0);
        std::vector<uint32_t> todo = {dfa_.start};
        std::vector<uint64_t> row((size_t)W);
        reachable_[dfa_.start] = 1;
        while (!todo.empty()) {
            const uint32_t q = todo.back();
            todo.pop_back();
            hip_check(hipMemcpy(row.data(), mask_ + (size_t)q * W, W * 8, hipMemcpyDeviceToHost), "D2H mask row");
            for (size_t w = 0; w < W; ++w)
                for (uint64_t bits = row[w]; bits; bits &= bits - 1) {
                    const uint32_t t = (uint32_t)(w * 64 + (size_t)__builtin_ctzll(bits));
                    const uint32_t next = step_token(q, t);
                    if (next < (uint32_t)S && !reachable_[next]) {
                        reachable_[next] = 1;
                        todo.push_back(next);
                    }
                }
        }
    } catch (...) {
        if (mask_) (void)hipFree(mask_);
        (void)hipFree(block_);
        throw;
    }
}

DeviceConstraint::~DeviceConstraint()
{
    (void)hipSetDevice(device_);
    if (mask_) (void)hipFree(mask_);
    if (block_) (void)hipFree(block_);
}

void DeviceConstraint::mask_row(uint32_t state, uint64_t* words_out) const
{
    if (state >= (uint32_t)dfa_.states()) throw InvalidConfig("constraint: state " + std::to_string(state) + " out of range");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipMemcpy(words_out, mask_ + (size_t)state * words(), (size_t)words() * 8, hipMemcpyDeviceToHost), "D2H mask");
}

ConstraintView DeviceConstraint::view(const std::vector<uint32_t>& stops) const
{
    if (stops.size() > (size_t)kConstraintMaxStops)
        throw InvalidConfig("a constrained call takes at most " + std::to_string(kConstraintMaxStops) + " stop ids, got " + std::to_string(stops.size()));
    ConstraintView v = {};
    v.mask = mask_;
    v.trans = trans_;
    v.flags = flags_;
    v.tok_off = off_;
    v.tok_bytes = bytes_;
    v.states = dfa_.states();
    v.vocab = vocab();
    v.words = words();
    v.n_stop = (int32_t)stops.size();
    for (size_t i = 0; i < stops.size(); ++i) v.stops[i] = stops[i];
    return v;
}

void DeviceConstraint::check_states(const std::vector<uint32_t>& stops) const
{
    if (stops.size() > (size_t)kConstraintMaxStops)
        throw InvalidConfig("a constrained call takes at most " + std::to_string(kConstraintMaxStops) + " stop ids, got " + std::to_string(stops.size()));
    std::vector<uint32_t> distinct;
    for (uint32_t s : stops)
        if (std::find(distinct.begin(), distinct.end(), s) == distinct.end()) distinct.push_back(s);
    for (int q = 0; q < dfa_.states(); ++q) {
        if (!reachable_[(size_t)q] || dfa_.closed[(size_t)q]) continue;
        if (dfa_.accepting[(size_t)q] && !stops.empty()) continue;
        uint32_t free_tokens = counts_[(size_t)q];
        for (uint32_t s : distinct)
            if (allows((uint32_t)q, s)) --free_tokens;  // (a stop id is governed by the accepting rule alone)
        if (free_tokens == 0)
            throw InvalidConfig("constraint: state " + std::to_string(q) + " allows no token of this vocabulary" +
                                (dfa_.accepting[(size_t)q] ? " and the call has no stop id to end on" : "") +
                                " (the pattern cannot be continued from there)");
    }
}

}  // namespace kjarni
