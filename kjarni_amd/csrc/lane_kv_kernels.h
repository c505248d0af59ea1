// Compact KV caches for the lock-step lanes (LlmModel::set_lane_kv_type): bf16 rows, or FP8 e4m3 (OCP e4m3fn, fp8_decode.h) rows with
// one f32 scale per (cache row, KV head).  Layout per layer and per K / V, lane-major: codes [lanes][lane_rows][kv] of 2 or 1 bytes
// and, for FP8, scales [lanes][lane_rows][n_kv_heads]; `lane_rows` (the rows a lane is allocated) is the one lane stride of both
// planes.  FP8 row of a head: scale = amax / 448, codes = RNE(x * (amax > 0 ? 448 / amax : 0)) clamped to +-448 before the convert
// (no code is NaN); a head row of zeros stores scale 0 and codes 0.  The scale pointers are not read for bf16 (may be null).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "llm_kernels.h"

namespace kjarni {

enum LaneKvType : int { LANE_KV_F32 = 0, LANE_KV_BF16 = 1, LANE_KV_F8_E4M3 = 2 };

// Bytes of one stored element (0 for a type that does not exist).
inline int lane_kv_elem_bytes(int type) { return type == LANE_KV_F32 ? 4 : type == LANE_KV_BF16 ? 2 : type == LANE_KV_F8_E4M3 ? 1 : 0; }

// launch_lane_rope_scatter / launch_lane_qk_norm_rope_scatter (llm_kernels.h) into compact planes: Q rotated in place in the staging
// rows, K rotated (rotate == 0: copied; the Qwen3 form: per-head RMSNorm first) and V copied, both encoded into row pos[lane] of the
// lane; frozen lanes and positions >= capacity write nothing.  The f32 value that is encoded is the f32 launchers' own, operation
// for operation, so a bf16 code is RNE of what an f32 lane would hold.  One workgroup per lane, one wave per head.  type: LANE_KV_BF16
// or LANE_KV_F8_E4M3; head_dim a multiple of 16 up to 128.
hipError_t launch_lane_rope_scatter_kv(int type, float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                       const float* cos_t, const float* sin_t, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                       int64_t lane_rows, int capacity, LaneStateRef state, int rotate, hipStream_t stream);
hipError_t launch_lane_qk_norm_rope_scatter_kv(int type, float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                               const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                               void* k_codes, void* v_codes, float* k_scale, float* v_scale, int64_t lane_rows, int capacity,
                                               LaneStateRef state, hipStream_t stream);

// Rows [0, rows) of every layer's f32 staging K and V ([rows][kv], what a prompt pass wrote) encoded into lane `lane` of the compact
// planes, one launch for all layers.  table[layer] lives in device memory: the staging pointers and the lane-0 plane pointers.
// 16-byte loads; 16-byte (bf16) or 8-byte (FP8) stores; a 16-lane row of a wave per (row, head).
struct LaneKvPackEntry {
    const float* src_k;
    const float* src_v;
    void* dst_k;
    void* dst_v;
    float* dst_k_scale;
    float* dst_v_scale;
};
hipError_t launch_lane_kv_pack(int type, const LaneKvPackEntry* table, int layers, int lane, int64_t lane_rows, int rows, int n_kv_heads,
                               int head_dim, hipStream_t stream);

// The lanes' ragged attention over compact planes: lane s attends to n = live[s] ? min(pos[s] + 1, capacity) : 0 keys of its own
// cache.  Grid (n_kv_heads * ceil(G / 8), splits, lanes), G = heads / n_kv_heads: a workgroup reads its key range of ONE KV head once
// and serves up to 8 of that head's query heads.  Writes launch_decode_attention's slabs [lanes, heads, splits, head_dim + 4]
// (scratch: decode_attention_scratch_floats) and merges them into ctx [lanes, ldc] with launch_decode_attention_combine (ctx null:
// the caller merges).  Range rule: ceil(n / splits) <= 512.  lane_attention_kv_accepts says whether the launcher takes the
// arguments (else hipErrorInvalidValue and nothing is launched): type bf16 or FP8, head_dim 16 / 32 / 64 / 128, heads a multiple of
// n_kv_heads, splits >= 1, ceil(capacity / splits) <= 512, lanes 1..64.
bool lane_attention_kv_accepts(int type, int lanes, int capacity, int heads, int n_kv_heads, int head_dim, int splits);
hipError_t launch_lane_attention_kv(int type, const float* q, int64_t ldq, int lanes, const void* k_codes, const void* v_codes,
                                    const float* k_scale, const float* v_scale, int64_t lane_rows, int capacity, int heads, int n_kv_heads,
                                    int head_dim, int splits, float* scratch, float* ctx, int64_t ldc, const int* lane_pos,
                                    const int* lane_live, hipStream_t stream);

}  // namespace kjarni
