// Launchers of fp8_kernels.hip: FP8 (OCP e4m3fn) matrices resident in HBM as their one-byte codes, with f32 scales
// (conventions of kernels.h: enqueue on `stream`, no allocation, no sync).  w[j, i] = decode(code[j, i]) * scale(j, i).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kjarni {

// The three scale layouts of the published checkpoints (the scale tensor's shape decides, fp8_scale_kind()).
enum { FP8_PER_TENSOR = 0, FP8_PER_CHANNEL = 1, FP8_BLOCK = 2 };
constexpr int kFp8Block = 128;  // block scales: one per 128 x 128 tile of the matrix
// The FP8 codes' entry in the per-type byte counts, beside the GGML type numbers (include/kjarni_hip.h:
// KJARNI_HIP_WEIGHT_TYPE_F8_E4M3; no GGML type in use here has this number).
constexpr int kFp8WeightType = 31;

// The kind of a scale tensor [scale_rows, scale_cols] beside a matrix [n, k]; -1: it fits none.
//   1 x 1 per tensor;  n x 1 per output channel;  ceil(n / 128) x k / 128 block (k % 128 == 0)
int fp8_scale_kind(int64_t n, int64_t k, int64_t scale_rows, int64_t scale_cols);

// One FP8 matrix [n, k] (row-major, HF row order; k % 16 == 0).
struct Fp8Mat {
    int n = 0, k = 0;
    const uint8_t* codes = nullptr;  // [n, k]
    const float* scale = nullptr;    // 1 | [n] | [ceil(n / 128), k / 128]
    int kind = FP8_PER_TENSOR;
};

// The projection over rows <= 8 activation rows, the weights streamed once:
//   F8_PLAIN   Y[0][r, c] = x[r] . W[0][c] (+ bias[c]) (+ R[r, c])
//   F8_QKV     the columns of W[0] | W[1] | W[2] from one read of the rows: W[0] -> Y[0] rows r, W[1] / W[2] -> Y[1] / Y[2] rows
//              row_off + r (*row_off_ptr when set: the cache rows of a captured step); bias over the concatenated columns
//   F8_SWIGLU  Y[0][r, c] = silu(x[r] . W[0][c]) * (x[r] . W[1][c])
// gamma: the rows are RMS-normalised on the way in, (x / sqrt(mean(x^2) + eps)) * gamma.
enum { F8_PLAIN = 0, F8_QKV = 1, F8_SWIGLU = 2 };
struct Fp8ProjArgs {
    int mode = F8_PLAIN;
    Fp8Mat W[3];
    const float* X = nullptr;
    int64_t ldx = 0;
    int rows = 0;
    const float* gamma = nullptr;
    float eps = 0.0f;
    const float* bias = nullptr;
    const float* R = nullptr;
    int64_t ldr = 0;
    float* Y[3] = {nullptr, nullptr, nullptr};
    int64_t ldy[3] = {0, 0, 0};
    int row_off = 0;
    const int* row_off_ptr = nullptr;
};
hipError_t launch_fp8_proj(const Fp8ProjArgs& a, hipStream_t stream);
// W dequantized into out [n, k] f32: decode(code) * scale, one f32 product per weight (the prompt route's scratch).
hipError_t launch_fp8_dequant(const Fp8Mat& W, float* out, hipStream_t stream);

// The prompt GEMM on the codes (fp8_gemm.hip): Y[M, N] = A[M, K] . W^T (+ bias) (+ R), N = W.n, K = W.k, on the bf16 matrix cores --
// the codes become exact bf16 operands in the tile loader, the f32 activations three exact bf16 pieces, the scale is applied in f32.
// launch_prefill_gemm's contract (llm_kernels.h): its tile order, its K-slice rule (prefill_gemm_launch_ksplit), its scratch layout
// and reduce kernel, R may alias Y, silu_gate as there.  Refused (hipErrorInvalidValue): K % 32, lda % 4, A or the codes not 16-byte
// aligned, block scales with K % 128.
hipError_t launch_prefill_gemm_fp8(const float* A, int64_t lda, const Fp8Mat& W, const float* bias, const float* R, int64_t ldr, float* Y,
                                   int64_t ldy, int M, hipStream_t stream, float* split_scratch = nullptr, float* silu_gate = nullptr);

}  // namespace kjarni
