// Launchers of moe_kernels.hip: the sparse (mixture-of-experts) FFN of Qwen3-MoE decoders (conventions of kernels.h: enqueue on
// `stream`, no allocation, no sync).  The rule, per row x (already RMS-normalised): router logits r = x . Wr^T, p = softmax(r)
// over all E experts, the k largest (on equal values the lower expert first), optionally renormalised to sum 1, then
//   y = R + sum_j w_j * down_{e_j}( silu(gate_{e_j} x) * up_{e_j} x ),   j = 0 .. k - 1 in slot order (largest weight first),
// with no float atomics anywhere: the order of every sum is fixed, two runs of one call give the same bits.
// The three expert matrices are stacks [E, Im, H] / [E, Im, H] / [E, H, Im], f32 or bf16, indexed by an expert id that every
// kernel reads from device memory (so a captured chain replays with whatever the router picks at replay time).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kjarni {

constexpr int MOE_MAX_EXPERTS = 256, MOE_MAX_TOPK = 8, MOE_TILE_ROWS = 64;

// softmax + top-k (+ renormalisation) over `rows` rows of router logits [rows, ldl]: ids [rows, k] (int32), weights [rows, k].
// The pick compares the logits (softmax is monotone; f32 probabilities that underflow to 0 would tie where the logits do not).
hipError_t launch_moe_route(const float* logits, int64_t ldl, int rows, int E, int k, int norm_topk, int32_t* ids, float* weights,
                            hipStream_t stream);

// Steps route, rows <= 8.  One slot is (row, j) of rows * k.
// gate/up: mid[slot, Im] = silu(gate_e . x) * (up_e . x), e = ids[slot]; x = X[row] (RMS-normalised by gamma first when non-null).
hipError_t launch_moe_gate_up(const float* X, int64_t ldx, int rows, const float* gamma, float eps, const int32_t* ids, int k, int E,
                              const void* gate, const void* up, int bf16, int H, int Im, float* mid, hipStream_t stream);
// down + combine + residual: Y[row] = R[row] + sum_j weights[row, j] * (down_{ids[row, j]} . mid[row * k + j]); R may be Y.
hipError_t launch_moe_down_combine(const float* mid, int rows, const int32_t* ids, const float* weights, int k, int E, const void* down,
                                   int bf16, int H, int Im, const float* R, int64_t ldr, float* Y, int64_t ldy, hipStream_t stream);

// Rows route.  The plan of S = rows * k slots, `moe_plan_ints(S, E)` ints: the slots sorted by expert (stable), the per-expert
// offsets [E + 1], a table of tiles (expert, first sorted slot, count <= 64) and the number of tiles.  All on the device: the grids
// of the kernels that read it are sized by moe_max_tiles(S, E), surplus tiles exit at once.
size_t moe_plan_ints(int S, int E);
int moe_max_tiles(int S, int E);
struct MoePlan {
    int32_t *sorted, *counts, *offsets, *tiles, *ntiles;
};
MoePlan moe_plan_at(int32_t* base, int S, int E);
hipError_t launch_moe_group(const int32_t* ids, int S, int E, int32_t* plan, hipStream_t stream);
// out[slot, N] over the tiles of the plan, A rows gathered through the sorted list (row of a slot = slot / a_div), W = stack + expert * N * K.
// W2 non-null: out = silu(A W^T) * (A W2^T) (gate / up); 64 x 64 tiles on v_mfma_f32_32x32x2_f32, bf16 stacks widened into LDS.  K % 32 == 0.
hipError_t launch_moe_grouped_gemm(const float* A, int64_t lda, int a_div, const int32_t* plan, int S, int E, const void* W, const void* W2,
                                   int bf16, int N, int K, float* out, hipStream_t stream);
// Y[row] = R[row] + sum_j weights[row, j] * y[row * k + j], j in order.
hipError_t launch_moe_combine(const float* y, const float* weights, int rows, int k, int H, const float* R, int64_t ldr, float* Y, int64_t ldy,
                              hipStream_t stream);

// The whole sparse FFN of `rows` rows, as the decoder's two layer bodies enqueue it.
struct MoeFfnArgs {
    const float* X = nullptr;  // [rows, ldx]
    int64_t ldx = 0;
    int rows = 0;
    const float* gamma = nullptr;  // non-null: RMSNorm(X, gamma, eps) feeds the router and the experts
    float eps = 0.0f;
    const void *router = nullptr, *gate = nullptr, *up = nullptr, *down = nullptr;  // [E, H], [E, Im, H], [E, Im, H], [E, H, Im]
    int bf16 = 0;
    int E = 0, k = 0, Im = 0, H = 0, norm_topk = 0;
    const float* R = nullptr;  // residual rows (may be Y)
    int64_t ldr = 0;
    float* Y = nullptr;
    int64_t ldy = 0;
    float* logits = nullptr;    // [rows, E] scratch
    int32_t* ids = nullptr;     // [rows, k]: the routing record
    float* weights = nullptr;   // [rows, k]
    float* mid = nullptr;       // [rows * k, Im] scratch
    // grouped route only
    float* xn = nullptr;        // [rows, H] scratch for the normalised rows (with gamma; X must then be contiguous, ldx == H)
    float* y = nullptr;         // [rows * k, H] scratch
    int32_t* plan = nullptr;    // moe_plan_ints(rows * k, E)
};
const char* moe_ffn_refusal(const MoeFfnArgs& a, bool grouped);  // null, or what the launchers refuse about these arguments
// rows <= 8: router (launch_llm_gemv, norm prologue) -> route -> gate/up -> down + combine: 4 launches.
hipError_t launch_moe_ffn_steps(const MoeFfnArgs& a, hipStream_t stream);
// any rows: [norm ->] router (launch_prefill_gemm) -> route -> group (2) -> gate/up GEMM -> down GEMM -> combine: 7 or 8 launches.
hipError_t launch_moe_ffn_grouped(const MoeFfnArgs& a, hipStream_t stream);

}  // namespace kjarni
