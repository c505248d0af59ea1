// What the scoring head kernels share (llm_kernels.hip: the f32 matrix-core head, the rows kernels and the merges;
// score_head_bf16.hip: the bf16 matrix-core head): the per-row running state, the slab partial both heads write and the
// merges read, and the argmax keys and top-k lists.  Device code only, everything inlined where it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_utils.h"
#include "llm_kernels.h"

namespace kjarni {

// the slab partials' geometry: row tiles of SC_BM rows, slab widths counted in tiles of SC_BN vocabulary columns
constexpr int SC_BM = 64, SC_BN = 64;

__device__ __forceinline__ unsigned long long argmax_key(float v, int idx)
{
    uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);  // -0.0 == +0.0 (partial_cmp): one key for both, the later index wins
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // larger float -> larger uint
    if (v != v) u = 0;                               // NaN lowest
    return ((unsigned long long)u << 32) | (uint32_t)idx;  // equal values: the LAST index wins (Iterator::max_by)
}

// What one slab of vocabulary tiles knows about one row.
struct ScorePartial {
    unsigned long long key;  // argmax_key of the slab's best logit (0: nothing seen)
    float mx;                // the slab's maximum
    float sm;                // sum of exp(x - mx) over the slab
    float tgt;               // the target's logit where the target lies in the slab, else 0
    float pad;
};

__device__ __forceinline__ float argmax_key_value(unsigned long long key)
{
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// (mx, sm) += (omx, osm): sums of exp(x - mx) brought to the common maximum.
__device__ __forceinline__ void score_combine(float& mx, float& sm, float omx, float osm)
{
    const float m = fmaxf(mx, omx);
    if (m == -INFINITY) return;  // both empty
    sm = sm * expf(mx - m) + osm * expf(omx - m);
    mx = m;
}

// Top-k lists: TOPK argmax_keys in descending order, every index static so that the list lives in registers; 0 marks an empty
// slot.  Keys of different columns differ, so "the TOPK largest keys" is one set whatever the order of the insertions.
constexpr int SC_TOPK = KJARNI_SCORE_TOPK_MAX;

template <int TOPK>
__device__ __forceinline__ void topk_insert(unsigned long long (&lst)[TOPK], unsigned long long kk)
{
    if (kk > lst[TOPK - 1]) {  // the one compare of the common path
#pragma unroll
        for (int j = TOPK - 1; j > 0; --j) lst[j] = kk > lst[j - 1] ? lst[j - 1] : (kk > lst[j] ? kk : lst[j]);
        lst[0] = kk > lst[0] ? kk : lst[0];
    }
}

// lst = the TOPK largest of lst and the list lane ^ off holds; every lane of a pair ends with the same list.
template <int TOPK>
__device__ __forceinline__ void topk_merge_lane(unsigned long long (&lst)[TOPK], int off)
{
    unsigned long long o[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) o[j] = __shfl_xor(lst[j], off, kWave);
#pragma unroll
    for (int j = 0; j < TOPK; ++j) topk_insert(lst, o[j]);
}

// The merges behind either head kernel (llm_kernels.hip): llm_score_merge_kernel over the partials P [row tile][slab][SC_BM],
// and llm_score_topk_merge_kernel over the key lists PK [row tile][slab][SC_TOPK][SC_BM] with the lse the former left.
hipError_t launch_score_merge(const ScorePartial* P, const uint32_t* targets, int m, int vocab, int slabs, int slab_tiles, float* logprob,
                              uint32_t* top, float* top_logprob, float* lse, hipStream_t stream);
hipError_t launch_score_topk_merge(const unsigned long long* PK, const float* lse, int m, int slabs, int top_k, uint32_t* topk_ids,
                                   float* topk_logprob, hipStream_t stream);

}  // namespace kjarni
