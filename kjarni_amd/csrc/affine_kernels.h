// Launchers of affine_kernels.hip: GGUF Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K matrices resident in HBM in the "affine-32" layout
// (described at the top of affine_kernels.hip), and the decode projection that serves them -- and Q8_0 in its own planes
// (quant_kernels.hip) where it shares a stage with them.  Conventions of kernels.h: enqueue on `stream`, no allocation, no sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "quant_kernels.h"

namespace kjarni {

bool ggml_affine_type(uint32_t type);  // Q4_0, Q4_1, Q5_0, Q5_1 or Q5_K
// Code width of a matrix the projection takes: 4 / 5 (affine-32), 8 (Q8_0), 0 for any other type.
int affine_code_bits(uint32_t type);
// Host side: raw GGUF blocks of an [n, k] matrix of an affine type -> plane[0] nibbles, plane[1] fifth bits (5-bit types),
// plane[2] the (a, b) pairs.  repack_ggml (quant_kernels.h) calls it for these types.
QPlanes repack_affine32(uint32_t type, const uint8_t* blocks, int n, int k);

// The projection over rows <= 8 activation rows, every matrix streamed once (W[i].k all equal, k % 32 == 0):
//   AF_PLAIN   Y[0][r, c] = x[r] . W[0][c] (+ bias[bias_off[0] + c]) (+ R[r, c])
//   AF_QKV     the columns of W[0] | W[1] | W[2] from one staging of the rows (a segment with n == 0 is absent): W[0] -> Y[0] rows r,
//              W[1] / W[2] -> Y[1] / Y[2] rows row_off + r (*row_off_ptr when set: the cache rows of a captured step); + bias[bias_off[s] + c]
//   AF_SWIGLU  Y[0][r, c] = silu(x[r] . W[0][c]) * (x[r] . W[1][c])
// gamma: the rows are RMS-normalised on the way in, x * (1 / sqrt(mean(x^2) + eps)) * gamma.  X 16-byte aligned, ldx % 4 == 0.
enum { AF_PLAIN = 0, AF_QKV = 1, AF_SWIGLU = 2 };
struct AffineProjArgs {
    int mode = AF_PLAIN;
    QMat W[3];
    const float* X = nullptr;
    int64_t ldx = 0;
    int rows = 0;
    const float* gamma = nullptr;
    float eps = 0.0f;
    const float* bias = nullptr;
    int bias_off[3] = {0, 0, 0};
    const float* R = nullptr;
    int64_t ldr = 0;
    float* Y[3] = {nullptr, nullptr, nullptr};
    int64_t ldy[3] = {0, 0, 0};
    int row_off = 0;
    const int* row_off_ptr = nullptr;
};
hipError_t launch_affine_proj(const AffineProjArgs& a, hipStream_t stream);
// W (an affine type) dequantized into out [n, k] f32: fmaf(a, q, b) per weight.
hipError_t launch_affine_dequant(const QMat& W, float* out, hipStream_t stream);
// The prompt GEMM on the affine-32 planes (affine_gemm.hip): Y[M, N] = A[M, K] . W^T (+ bias) (+ R), N = W.n, K = W.k, on the bf16
// matrix cores -- the codes, less 8 / 16, become exact bf16 integers in the tile loader, the f32 activations three exact bf16 pieces,
// (a, b) of every run is applied in f32.  launch_prefill_gemm_ggml's contract (quant_kernels.h): tile order, K-slice rule
// (prefill_gemm_launch_ksplit), scratch layout and reduce kernel, R may alias Y, silu_gate as there.  Refused (hipErrorInvalidValue):
// a type that is not one of the five, K % 32 (K % 256 for Q5_K), lda % 4, A or a plane not 16-byte aligned, a 5-bit type without
// q2, a gate with ldy != N or N % 4.
hipError_t launch_prefill_gemm_affine(const float* A, int64_t lda, const QMat& W, const float* bias, const float* R, int64_t ldr, float* Y,
                                      int64_t ldy, int M, hipStream_t stream, float* split_scratch = nullptr, float* silu_gate = nullptr);
// Embedding rows ids[0..n) of an affine-type table [vocab, hidden], dequantized; an id >= vocab gives zeros.
hipError_t launch_affine_embed(const uint32_t* ids, int n, const QMat& table, float* out, hipStream_t stream);

}  // namespace kjarni
