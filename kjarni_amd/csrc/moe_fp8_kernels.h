// Launchers of moe_fp8_kernels.hip: the sparse FFN of moe_kernels.h over expert stacks that stay FP8 (OCP e4m3fn) codes in HBM
// (conventions of kernels.h: enqueue on `stream`, no allocation, no sync).  w_e[j, i] = decode(code_e[j, i]) * scale_e(j, i); the
// rule, the slot order and the contract of moe_kernels.h hold: no float atomics, every sum has one order, two runs give the same
// bits.  The expert id of a slot is read on the device, so the base of a matrix is stack + id * n * k (codes) and scale + id *
// (the per-expert extent of the scales): a captured chain replays with whatever the router picks.  No f32 or bf16 copy of an
// expert matrix is made: the steps route streams the codes, the rows route turns them into bf16 operands in the tile loader.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp8_kernels.h"
#include "moe_kernels.h"

namespace kjarni {

// One stack [E, n, k] of codes with its f32 scales [E, extent], one kind for the whole stack (FP8_PER_TENSOR / _CHANNEL / _BLOCK).
struct MoeFp8Stack {
    const uint8_t* codes = nullptr;
    const float* scale = nullptr;
    int kind = FP8_PER_TENSOR;
};
// floats of scale per expert: 1, n, or ceil(n / 128) * (k / 128); 0 for an unknown kind
int64_t moe_fp8_scale_extent(int kind, int64_t n, int64_t k);

// Steps route, rows <= 8: mid[slot, Im] = silu(gate_e . x) * (up_e . x), e = ids[slot]; x = X[row], RMS-normalised when gamma.
// H % 32 == 0, Im % 32 == 0; block scales: H % 128 == 0.
hipError_t launch_moe_fp8_gate_up(const float* X, int64_t ldx, int rows, const float* gamma, float eps, const int32_t* ids, int k, int E,
                                  const MoeFp8Stack& gate, const MoeFp8Stack& up, int H, int Im, float* mid, hipStream_t stream);
// Y[row] = R[row] + sum_j weights[row, j] * (down_{ids[row, j]} . mid[row * k + j]), j in slot order; R may be Y.  Block scales: Im % 128 == 0.
hipError_t launch_moe_fp8_down_combine(const float* mid, int rows, const int32_t* ids, const float* weights, int k, int E,
                                       const MoeFp8Stack& down, int H, int Im, const float* R, int64_t ldr, float* Y, int64_t ldy,
                                       hipStream_t stream);
// Rows route: launch_moe_grouped_gemm on the codes, over the same device plan.  out[slot, N] = A[slot / a_div] . W_e^T, or with W2:
// silu(A W_e^T) * (A W2_e^T).  64 x 64 tiles on v_mfma_f32_32x32x16_bf16: A as three exact bf16 planes, the codes as exact bf16.
// K % 32 == 0; block scales: K % 128 == 0.
hipError_t launch_moe_fp8_grouped_gemm(const float* A, int64_t lda, int a_div, const int32_t* plan, int S, int E, const MoeFp8Stack& W,
                                       const MoeFp8Stack* W2, int N, int K, float* out, hipStream_t stream);

// The whole sparse FFN: MoeFfnArgs with the three stacks here (its gate / up / down stay null; router, bf16: the router matrix).
struct MoeFp8FfnArgs {
    MoeFfnArgs base;
    MoeFp8Stack gate, up, down;  // [E, Im, H], [E, Im, H], [E, H, Im]
};
const char* moe_fp8_ffn_refusal(const MoeFp8FfnArgs& a, bool grouped);  // moe_ffn_refusal's, and what the codes add
// router -> route -> gate/up -> down + combine: 4 launches
hipError_t launch_moe_fp8_ffn_steps(const MoeFp8FfnArgs& a, hipStream_t stream);
// [norm ->] router -> route -> group (2) -> gate/up GEMM -> down GEMM -> combine: 7 or 8 launches
hipError_t launch_moe_fp8_ffn_grouped(const MoeFp8FfnArgs& a, hipStream_t stream);

}  // namespace kjarni
