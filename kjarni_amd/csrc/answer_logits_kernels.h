// Answer logits (LlmModel::answer_logits_batch): the kernel that turns a sequence's last hidden row into the logits of a few
// chosen tokens without the vocabulary head (answer_logits_kernels.hip).  The plan is answer_plan_host, score_batch_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kjarni {

constexpr int kAnswerMaxTargets = 8;

// out[j, t] = dot(norm(x[src[j], :hidden]), head[targets[t], :hidden]) for j < n, t < n_targets (1 .. kAnswerMaxTargets), out rows
// n_targets floats apart.  beta null: RMSNorm with rmsnorm_kernel's summation order; beta given: launch_layernorm's arithmetic.
// head: [*, hidden] row-major, f32 or bf16 (head_is_bf16), rows hidden elements apart; every targets[t] must be a row of it (the
// caller checks).  One workgroup per output row; hidden 1 .. 16384, any ldx >= hidden, any alignment of x and head that their
// element type allows.  Reads row src[j] of x, gamma (and beta) and the targeted head rows, nothing else.
hipError_t launch_answer_logits(const float* x, int64_t ldx, const int32_t* src, int n, int hidden, const float* gamma, const float* beta,
                                float eps, const void* head, int head_is_bf16, const uint32_t* targets, int n_targets, float* out,
                                hipStream_t stream);

}  // namespace kjarni
