// Launchers of quant_kernels.hip: GGUF Q8_0 / Q4_K / Q6_K matrices resident in HBM (conventions of kernels.h: enqueue on
// `stream`, no allocation, no sync).  The device layout is described at the top of quant_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace kjarni {

// One quantized matrix [n, k] (row-major, HF row order) in its device layout.
struct QMat {
    uint32_t type = 0;  // GGML_Q8_0 / GGML_Q4_K / GGML_Q6_K (gguf.h)
    int n = 0, k = 0;
    const void* q = nullptr;   // quants plane
    const void* q2 = nullptr;  // Q6_K: high-bits plane
    const void* s = nullptr;   // f32 scales plane
    const void* s2 = nullptr;  // Q6_K: int8 sub-block scales plane
};

// Host side: raw GGUF blocks of an [n, k] matrix -> the device planes (q, q2, s, s2; unused ones empty).
struct QPlanes {
    std::vector<uint8_t> plane[4];
};
QPlanes repack_ggml(uint32_t type, const uint8_t* blocks, int n, int k);
bool ggml_matrix_type(uint32_t type);  // Q8_0, Q4_K or Q6_K

// Y[r, j] = sum_i X[r, i] W[j, i] (+ bias[j]) (+ R[r, j]) for r < rows <= 8: QF_PLAIN of launch_qfused (below).
//   Q8_0 / Q4_K, and Q6_K with Xq == null: f32 activations x dequantized weights
//   Q6_K with Xq: Q8_K activation codes (launch_q8k_quantize) x the 6-bit codes in integers per 256-block, then d_w d_a
struct QGemvArgs {
    QMat W;
    const float* X = nullptr;
    int64_t ldx = 0;
    const int8_t* Xq = nullptr;  // [rows, k] codes
    const float* Xd = nullptr;   // [rows, k / 256] scales
    int rows = 0;
    const float* bias = nullptr;
    const float* R = nullptr;
    int64_t ldr = 0;
    float* Y = nullptr;
    int64_t ldy = 0;
};
hipError_t launch_qgemv(const QGemvArgs& a, hipStream_t stream);
// The decode step's fused launches (one wave per job of two output columns, weights streamed once):
//   QF_PLAIN   Y[0][r, c] = sum_i x[r, i] W[0][c, i] (+ bias) (+ R[r, c])                      jobs = ceil(n / 2)
//   QF_QKV     Q | K | V of W[0..2] (each its own type) from one read of the rows: Q -> Y[0] rows r, K / V -> Y[1] / Y[2] rows
//              row_off + r (the caches), + bias (bias_off per segment); Q and K rotated (RoPE, cos/sin [pos, head_dim/2]) in
//              the epilogue: a job is the pair (i, i + head_dim/2) of one head                        jobs = sum of n_s / 2
//   QF_SWIGLU  Y[0][r, c] = silu(x . W[0][c]) * (x . W[1][c])                                          jobs = n
// gamma: the rows are RMS-normalised on the fly (x * (1 / rms) * gamma).  Xq / Xd: Q8_K codes of the (normalised) rows,
// used by Q6_K matrices (linears); without them a Q6_K matrix takes f32 activations (the tied head).
enum { QF_PLAIN = 0, QF_QKV = 1, QF_SWIGLU = 2 };
struct QFusedArgs {
    int mode = QF_PLAIN;
    QMat W[3];
    int seg_jobs[3] = {0, 0, 0};
    int jobs = 0, k = 0;
    const float* X = nullptr;
    int64_t ldx = 0;
    int rows = 0;
    const float* gamma = nullptr;
    float eps = 0.0f;
    const int8_t* Xq = nullptr;
    const float* Xd = nullptr;
    const float* bias = nullptr;
    int bias_off[3] = {0, 0, 0};
    const float* R = nullptr;
    int64_t ldr = 0;
    float* Y[3] = {nullptr, nullptr, nullptr};
    int64_t ldy[3] = {0, 0, 0};
    int row_off = 0;
    const int* row_off_ptr = nullptr;
    int head_dim = 0;
    const float* cos_t = nullptr;
    const float* sin_t = nullptr;
};
hipError_t launch_qfused(const QFusedArgs& a, hipStream_t stream);
// RMSNorm (gamma set) and / or Q8_K quantization of rows [rows, k] in one launch (one workgroup per row): normalised rows to
// xn (may be null), codes / scales (may be null).  Normalisation as rmsnorm_kernel: (x / rms) * gamma.
hipError_t launch_qprep(const float* X, int64_t ldx, int rows, int k, const float* gamma, float eps, float* xn, int8_t* codes, float* scales,
                        hipStream_t stream);
// Q8_K quantization of rows of X [rows, k] (k % 256 == 0; kernels/quantize.rs:57-126): codes [rows, k], scales [rows, k / 256];
// deq (optional, [rows, k]): the codes times their scale (the prompt route feeds these to the f32 GEMM); codes / scales may be
// null when only deq is wanted.
hipError_t launch_q8k_quantize(const float* X, int64_t ldx, int rows, int k, int8_t* codes, float* scales, float* deq, hipStream_t stream);
// W dequantized into out [n, k] f32 (the prompt route's f32 scratch).
hipError_t launch_qdequant(const QMat& W, float* out, hipStream_t stream);
// Embedding rows ids[0..n) of the table [vocab, hidden], dequantized; an id >= vocab gives zeros.
hipError_t launch_qembed(const uint32_t* ids, int n, const QMat& table, float* out, hipStream_t stream);

}  // namespace kjarni
