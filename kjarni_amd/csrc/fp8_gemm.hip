// The prompt GEMM over FP8 (OCP e4m3fn) weights on the bf16 matrix cores: Y[M, N] = A . W^T with the one-byte codes read from HBM
// and turned into bf16 operands on the way into LDS -- no f32 copy of the matrix through HBM (launch_fp8_dequant + the f32 GEMM is
// the route this replaces where the decoder's switch is on).
//
// An e4m3fn code has 3 mantissa bits and exponents 2^-9 .. 2^8 (448 the largest value): its value is a bf16 number exactly, so the
// weight operand is exact.  The f32 activations are three exact bf16 pieces (bf16_split.h), as in prefill_gemm_bf16w_kernel
// (gemm_split.hip), whose tile order, K slices, partial layout and MFMA loop this kernel shares: three bf16 MFMAs per 16 columns of
// K, every product exact, f32 accumulation.  Only the scale is left, and it stays f32 (folding it into the bf16 operand would round):
//   per tensor / per channel   acc * scale[col] in the epilogue -- before the bias, and before a partial tile goes to the split
//                              scratch, so that prefill_splitk_reduce_kernel adds finished products
//   block (128 x 128)          a 64-column tile starts at a multiple of 64 and so lies inside one row of blocks; along K the MFMAs
//                              fill a block accumulator that is folded into the tile's, total += s * blk, whenever the ABSOLUTE k
//                              reaches a multiple of 128 (a K slice may begin in the middle of a block: K = 384 in two slices of 192)
//                              and at the end of the slice
// Its own translation unit because, like gemm_split.hip, it is compiled with -fno-slp-vectorize (the split's subtractions must not
// become packed f32 adds beside the MFMAs); fp8_kernels.hip keeps the flags its decode-step kernels were measured with.
#include <hip/hip_runtime.h>

#include "bf16_split.h"
#include "device_utils.h"
#include "fp8_kernels.h"
#include "llm_kernels.h"

namespace kjarni {

namespace {

constexpr int FG_BM = 64, FG_BN = 64, FG_BK = 32;
constexpr int FG_PLANE = 64 * 32;  // bf16 per plane: 64 rows x 64 bytes, the four 16-byte chunks of a row swizzled by (row >> 2) & 3

// Eight codes (two dwords, code j in byte j) as eight bf16 in the same order: v_cvt_scalef32_pk_bf16_fp8 with scale 1.0, one
// instruction per pair of codes (v_cvt_pk_f32_fp8 and a byte permute to keep the high halves is the same result in twice as many).
// Every e4m3fn value is a bf16 number, so the conversion has nothing to round; the scale operand stays 1.0 -- a matrix's real scale
// is applied in f32 (above).
__device__ __forceinline__ u32x4 fp8x8_to_bf16x8(u32x2 c)
{
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        o[2 * d] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, false));     // codes 4d, 4d + 1
        o[2 * d + 1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[d], 1.0f, true));  // codes 4d + 2, 4d + 3
    }
    return o;
}

// One workgroup per (64 x 64 tile, K slice): 256 threads, four waves of one 32 x 32 tile each, LDS double-buffered as
// [stage][A1 | A2 | A3 | W].  scale: FP8_PER_TENSOR [1], FP8_PER_CHANNEL [N], FP8_BLOCK [ceil(N / 128)][scale_cols].
template <bool RESIDUAL, int KIND>
__global__ __launch_bounds__(256) void prefill_gemm_fp8w_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ W,
                                                                const float* __restrict__ scale, int scale_cols,
                                                                const float* __restrict__ bias, const float* R, int64_t ldr, float* Y,
                                                                int64_t ldy, int M, int N, int K, int m_tiles, int ksplit,
                                                                float* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) uint16_t sp[2][4 * FG_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    // the tile order of prefill_gemm_kernel: consecutive tiles on one XCD
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned bid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    const int ks = (int)(bid0 % (unsigned)ksplit);
    const unsigned bid = bid0 / (unsigned)ksplit;
    const int m0 = (int)(bid % (unsigned)m_tiles) * FG_BM;
    const int n0 = (int)(bid / (unsigned)m_tiles) * FG_BN;
    const int k_len = K / ksplit, k_begin = ks * k_len;

    const int a_row = tid >> 3, a_c4 = tid & 7, b_row = tid >> 2, b_c = tid & 3;
    const float* a_ptr[2];
    int stA[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = a_row + 32 * i;
        a_ptr[i] = A + (int64_t)min(m0 + row, M - 1) * lda + a_c4 * 4 + k_begin;  // rows at or past M: the last row again, never stored
        stA[i] = row * 32 + (((a_c4 >> 1) ^ ((row >> 2) & 3)) * 2 + (a_c4 & 1)) * 4;
    }
    const uint8_t* b_ptr = W + (int64_t)min(n0 + b_row, N - 1) * K + b_c * 8 + k_begin;  // eight codes per lane and K step
    const int stW = 3 * FG_PLANE + b_row * 32 + (b_c ^ ((b_row >> 2) & 3)) * 8;
    f32x4 ga[2];
    u32x2 gw;
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
        gw = *reinterpret_cast<const u32x2*>(b_ptr + k0);
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p1, p2, p3;
            sp_split(ga[i], p1, p2, p3);
            *reinterpret_cast<u32x2*>(&sp[stage][stA[i]]) = p1;
            *reinterpret_cast<u32x2*>(&sp[stage][FG_PLANE + stA[i]]) = p2;
            *reinterpret_cast<u32x2*>(&sp[stage][2 * FG_PLANE + stA[i]]) = p3;
        }
        *reinterpret_cast<u32x4*>(&sp[stage][stW]) = fp8x8_to_bf16x8(gw);  // decoded once per element, here
    };
    f32x16 acc, total;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = total[r] = 0.0f;
    const int nk = k_len / FG_BK;
    const int fsw = (l31 >> 2) & 3;
    const int fa = (wr * 32 + l31) * 32, fb = 3 * FG_PLANE + (wc * 32 + l31) * 32;
    const float* brow = scale + (int64_t)(n0 >> 7) * scale_cols;  // (block scales: this tile's row of blocks)
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * FG_BK);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int ch = ((kb * 2 + half) ^ fsw) * 8;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&sp[cur][fb + ch]);
#pragma unroll
            for (int p = 2; p >= 0; --p) {  // the smallest piece first
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sp[cur][p * FG_PLANE + fa + ch]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
        }
        if (KIND == FP8_BLOCK) {
            const int k_end = k_begin + (kt + 1) * FG_BK;  // absolute: the columns of K done so far end here
            if ((k_end & (kFp8Block - 1)) == 0 || kt + 1 == nk) {
                const float s = brow[(k_end - 1) >> 7];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    total[r] += s * acc[r];
                    acc[r] = 0.0f;
                }
            }
        }
        if (kt + 1 < nk) store(cur ^ 1);
        __syncthreads();
    }
    const int col = n0 + wc * 32 + l31;
    if (col < N) {
        if (KIND == FP8_BLOCK) {
            acc = total;
        } else {
            const float sc = KIND == FP8_PER_CHANNEL ? scale[col] : scale[0];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] *= sc;
        }
        if (ksplit > 1) {
            float* out = P + (int64_t)ks * M * N;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * 32 + acc_row(r, half);
                if (row < M) out[(int64_t)row * N + col] = acc[r];
            }
            return;
        }
        const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wr * 32 + acc_row(r, half);
            if (row < M) {
                float v = acc[r] + bv;
                if (RESIDUAL) v += R[(int64_t)row * ldr + col];
                Y[(int64_t)row * ldy + col] = v;
            }
        }
    }
}

}  // namespace

hipError_t launch_prefill_gemm_fp8(const float* A, int64_t lda, const Fp8Mat& W, const float* bias, const float* R, int64_t ldr, float* Y,
                                   int64_t ldy, int M, hipStream_t stream, float* split_scratch, float* silu_gate)
{
    const int N = W.n, K = W.k;
    if (M <= 0 || N <= 0) return hipSuccess;
    if (K <= 0 || K % FG_BK || lda % 4 || (reinterpret_cast<uintptr_t>(A) & 15) || !W.codes || !W.scale || (reinterpret_cast<uintptr_t>(W.codes) & 15))
        return hipErrorInvalidValue;
    if (W.kind != FP8_PER_TENSOR && W.kind != FP8_PER_CHANNEL && W.kind != FP8_BLOCK) return hipErrorInvalidValue;
    if (W.kind == FP8_BLOCK && K % kFp8Block) return hipErrorInvalidValue;
    if (silu_gate && (ldy != N || (N & 3) || (reinterpret_cast<uintptr_t>(silu_gate) & 15))) return hipErrorInvalidValue;
    const int m_tiles = (M + FG_BM - 1) / FG_BM, n_tiles = (N + FG_BN - 1) / FG_BN;
    const int ksplit = prefill_gemm_launch_ksplit(bias, R, ldr, Y, ldy, M, N, K, split_scratch);  // (slices of a multiple of 32 columns)
    const dim3 grid((unsigned)(m_tiles * n_tiles * ksplit));
    const int scale_cols = W.kind == FP8_BLOCK ? K / kFp8Block : 0;
#define KJ_FG(RES, KIND)                                                                                                               \
    hipLaunchKernelGGL((prefill_gemm_fp8w_kernel<RES, KIND>), grid, dim3(256), 0, stream, A, lda, W.codes, W.scale, scale_cols, bias, R, ldr, \
                       Y, ldy, M, N, K, m_tiles, ksplit, split_scratch)
#define KJ_FG_KIND(KIND)    \
    do {                    \
        if (R) KJ_FG(true, KIND);  \
        else KJ_FG(false, KIND);   \
    } while (0)
    if (W.kind == FP8_BLOCK) KJ_FG_KIND(FP8_BLOCK);
    else if (W.kind == FP8_PER_CHANNEL) KJ_FG_KIND(FP8_PER_CHANNEL);
    else KJ_FG_KIND(FP8_PER_TENSOR);
#undef KJ_FG_KIND
#undef KJ_FG
    if (ksplit > 1) return launch_prefill_splitk_reduce(split_scratch, ksplit, bias, R, ldr, Y, ldy, M, N, silu_gate, stream);
    if (silu_gate) return launch_swiglu_mul(silu_gate, Y, (size_t)M * N, stream);
    return hipGetLastError();
}

}  // namespace kjarni
