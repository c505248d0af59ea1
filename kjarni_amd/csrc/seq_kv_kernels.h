// The single-sequence KV cache in bf16 or FP8 e4m3 (LlmModel::set_kv_type): lane_kv_kernels.h's codes, scale rule and layout with a lane
// count of 1 -- per layer and per K / V codes [rows][kv] of 2 or 1 bytes and, for FP8, scales [rows][n_kv_heads].  The one-row decode
// step runs the lane kernels with one lane; what is new here serves blocks of rows at consecutive positions (a prompt chunk, the <= 8
// verify rows of speculative decoding): a row-indexed encoding scatter and a causal attention over the codes on the bf16 matrix cores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_kv_kernels.h"

namespace kjarni {

// Row r of the block sits at position p = (base_ptr ? *base_ptr : base) + r.  Its Q heads (row r of q, ldq floats apart) are rotated in
// place, its K heads (row r of k) rotated and its V heads (row r of v) copied, both encoded into cache row p; gamma_q / gamma_k
// non-null: the Qwen3 per-head RMSNorm of Q and K first; rotate == 0 (GPT-2): Q untouched, K copied.  The arithmetic up to the
// encoded f32 value is rope_kernel's / head_norm_rope's (llm_kernels.hip), expression for expression, so a bf16 code is RNE of what
// the f32 cache would hold.  Rows with p >= capacity write nothing.  One workgroup per row, one wave per head; type bf16 or FP8,
// head_dim a multiple of 16 up to 128.
hipError_t launch_seq_kv_scatter(int type, float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int rows,
                                 int n_heads, int n_kv_heads, int head_dim, const float* gamma_q, const float* gamma_k, float eps,
                                 const float* cos_t, const float* sin_t, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                 int base, const int* base_ptr, int capacity, int rotate, hipStream_t stream);

// launch_prefill_attention's contract over code planes: query row r (row r of q, heads * head_dim floats) at position base + r
// (base_ptr: *base_ptr + r) attends to cache rows [0, base + r].  Grid (n_kv_heads * ceil(G / 8) * row blocks, splits): one wave owns
// one KV head and a 32-row M tile of (query row, group head) pairs, so a key tile is read once for the whole group; S^T = K Q^T and
// O^T = V^T P^T on v_mfma_f32_32x32x16_bf16 with Q and P split into three exact bf16 planes (every product exact, f32 accumulation in
// a fixed order, no atomics).  The key range of a tile is cut into `splits` slabs [rows, heads, splits, head_dim + 4]
// (decode_attention_scratch_floats(rows, heads, head_dim, splits) floats of scratch) that launch_decode_attention_combine merges
// into ctx [rows, ldc] (ctx null: the caller merges).  seq_attention_kv_accepts says whether the launcher takes the arguments (else
// hipErrorInvalidValue and nothing is launched): type bf16 or FP8, head_dim 16 / 32 / 64 / 128, heads a multiple of n_kv_heads,
// rows >= 1, base >= 0, base + rows <= capacity, splits >= 1.
bool seq_attention_kv_accepts(int type, int rows, int base, int capacity, int heads, int n_kv_heads, int head_dim, int splits);
hipError_t launch_seq_attention_kv(int type, const float* q, int64_t ldq, int rows, const void* k_codes, const void* v_codes,
                                   const float* k_scale, const float* v_scale, int base, const int* base_ptr, int capacity, int heads,
                                   int n_kv_heads, int head_dim, int splits, float* scratch, float* ctx, int64_t ldc, hipStream_t stream);

}  // namespace kjarni
