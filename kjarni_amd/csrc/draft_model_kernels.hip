// The kernels of draft-model speculative decoding (llm.cpp: LlmModel::enqueue_draft): the begin of a round and the hand-off of
// the drafter's argmax into the target's verify block.  Plain vector stores, no scratch memory, no LDS beyond one reduction
// array; everything else on the chain is an existing kernel of the two models.
#include "draft_model_kernels.h"

#include "llm_kernels.h"

namespace kjarni {

namespace {

constexpr int DM_THREADS = 256, DM_WAVE = 64, DM_MAX_ROWS = 8;

// One wave.  Lane r < rows writes ids[r]; lane 0 the state and the drafter's position; lanes 0 / 1 the drafter's two ids.
__global__ __launch_bounds__(DM_WAVE) void draft_begin_kernel(const int32_t* __restrict__ T, int hist_cap, LlmLookupState* __restrict__ st,
                                                              int rows, uint32_t* __restrict__ drafter_ids, int* __restrict__ drafter_pos,
                                                              uint32_t* __restrict__ ids)
{
    const int tid = threadIdx.x;
    int n = st->n;
    n = n < 2 ? 2 : (n > hist_cap ? hist_cap : n);  // (hist_cap >= 2: the launcher checks)
    const uint32_t last = (uint32_t)T[n - 1];
    if (tid < rows) ids[tid] = last;
    if (rows > 1 && tid < 2) drafter_ids[tid] = tid == 0 ? (uint32_t)T[n - 2] : last;
    if (tid == 0) {
        st->m = rows - 1;
        if (rows > 1) *drafter_pos = n - 2;
    }
}

// launch_argmax's key: larger float -> larger key, NaN lowest, -0.0 == +0.0, equal values: the later index wins.
__device__ __forceinline__ unsigned long long draft_key(float v, int idx)
{
    uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (v != v) u = 0;
    return ((unsigned long long)u << 32) | (uint32_t)idx;
}

__global__ __launch_bounds__(DM_THREADS) void draft_argmax_kernel(const float* __restrict__ logits, int vocab,
                                                                  unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long red[DM_THREADS / DM_WAVE];
    unsigned long long key = 0ull;
    for (int i = blockIdx.x * DM_THREADS + threadIdx.x; i < vocab; i += gridDim.x * DM_THREADS) {
        const unsigned long long k = draft_key(logits[i], i);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int off = DM_WAVE / 2; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, DM_WAVE);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & (DM_WAVE - 1)) == 0) red[threadIdx.x / DM_WAVE] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DM_THREADS / DM_WAVE; ++w) key = red[w] > key ? red[w] : key;
        atomicMax(best, key);
    }
}

// Publishes the drafter's pick where the next drafter step and the target's verify block read it, re-zeroes the accumulator
// and moves the drafter's position past the rows its pass wrote.
__global__ void draft_handoff_kernel(unsigned long long* __restrict__ best, uint32_t* __restrict__ id_out, int* __restrict__ drafter_pos,
                                     int advance)
{
    if (threadIdx.x != 0) return;
    *id_out = (uint32_t)(*best & 0xFFFFFFFFull);
    *best = 0ull;
    *drafter_pos += advance;
}

}  // namespace

hipError_t launch_draft_begin(const int32_t* history, int hist_cap, LlmLookupState* state, int rows, uint32_t* drafter_ids, int* drafter_pos,
                              uint32_t* ids, hipStream_t stream)
{
    if (rows < 1 || rows > DM_MAX_ROWS || hist_cap < 2 || !history || !state || !ids || (rows > 1 && (!drafter_ids || !drafter_pos)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(draft_begin_kernel, dim3(1), dim3(DM_WAVE), 0, stream, history, hist_cap, state, rows, drafter_ids, drafter_pos, ids);
    return hipGetLastError();
}

hipError_t launch_draft_handoff(const float* logits, int vocab, unsigned long long* best_scratch, uint32_t* id_out, int* drafter_pos,
                                int advance, hipStream_t stream)
{
    if (vocab < 1 || advance < 0 || !logits || !best_scratch || !id_out || !drafter_pos) return hipErrorInvalidValue;
    int blocks = (vocab + 2047) / 2048;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(draft_argmax_kernel, dim3((unsigned)blocks), dim3(DM_THREADS), 0, stream, logits, vocab, best_scratch);
    hipLaunchKernelGGL(draft_handoff_kernel, dim3(1), dim3(DM_WAVE), 0, stream, best_scratch, id_out, drafter_pos, advance);
    return hipGetLastError();
}

}  // namespace kjarni
