// The prompt GEMM over GGUF quantized weights (Q8_0 / Q4_K / Q6_K, the device planes of quant_kernels.hip) on the bf16 matrix cores:
// Y[M, N] = A . W^T with the code bytes read from HBM and unpacked into bf16 integer operands on the way into LDS -- no f32 or bf16
// copy of the matrix through HBM (launch_qdequant + the f32 GEMM is the route this replaces where the decoder's switch is on).
//
// The integer codes are bf16 numbers exactly (Q8_0 -128 .. 127, Q4_K 0 .. 15, Q6_K q - 32 in -32 .. 31) and the f32 activations are
// three exact bf16 pieces (bf16_split.h), so every matrix-core product is exact, as in prefill_gemm_fp8w_kernel (fp8_gemm.hip), whose
// tile order, K slices, partial layout, LDS swizzle and MFMA loop this kernel shares.  The scales stay f32 and are folded per
// sub-block: in a 32 x 32 accumulator a lane owns one output column, i.e. one weight row, so a sub-block's scale is one scalar per
// lane and the fold is total[r] += s * acc[r]; acc[r] = 0 --
//   Q8_0   d per 32 columns of K: one fold per 32-wide K step
//   Q4_K   (d*sc_j) and (dmin*m_j) per 32-element sub-block, w = (d*sc_j) q - (dmin*m_j): one fold per K step,
//          total += (d*sc_j) acc - (dmin*m_j) rowsum, rowsum the sum of the activation row over the step's 32 columns -- formed in
//          the A loader (the eight lanes that hold a row's slice reduce among themselves) and kept in LDS beside the stage, where a
//          lane reads its 16 accumulator rows as four 16-byte words
//   Q6_K   d * sc_j per 16-element sub-block: one fold per MFMA group of 16 columns of K, two per K step
// The scale of a step is indexed with the ABSOLUTE k (a K slice is a multiple of 32 columns and may begin inside a 256-block) and is
// loaded a tile ahead, with the codes.
//
// The K tile is 32 columns for every type.  A Q4_K chunk's 32 bytes hold 64 elements (low nibbles k .. k + 31, high nibbles
// k + 32 .. k + 63), so each chunk byte is loaded twice, by two consecutive K steps of the same workgroup; a 64-wide K tile would load
// it once but doubles the stage (64 KiB of LDS for two stages, one workgroup per CU less) and gives Q4_K a loop of its own.  The
// second load is 8 bytes per lane from a line the step before has just brought in -- the same 8 bytes per lane and step the FP8
// kernel loads -- so the 32-wide tile is kept.
//
// One kernel instance per (type, residual): the unpack and the fold of a type are compiled alone (DESIGN section 6 has what one
// kernel with every type's path cost the GEMV).  Its own translation unit because, like gemm_split.hip and fp8_gemm.hip, it is
// compiled with -fno-slp-vectorize.
#include <hip/hip_runtime.h>

#include "bf16_split.h"
#include "device_utils.h"
#include "gguf.h"
#include "llm_kernels.h"
#include "quant_kernels.h"

namespace kjarni {

namespace {

constexpr int GG_BM = 64, GG_BN = 64, GG_BK = 32;
constexpr int GG_PLANE = 64 * 32;  // bf16 per plane: 64 rows x 64 bytes, the four 16-byte chunks of a row swizzled by (row >> 2) & 3

// Four small integers as four bf16 (two dwords): an integer of at most 8 significant bits is a bf16 number, the high half of its f32.
__device__ __forceinline__ u32x2 ints4_to_bf16(float f0, float f1, float f2, float f3)
{
    return u32x2{(__builtin_bit_cast(uint32_t, f0) >> 16) | (__builtin_bit_cast(uint32_t, f1) & 0xffff0000u),
                 (__builtin_bit_cast(uint32_t, f2) >> 16) | (__builtin_bit_cast(uint32_t, f3) & 0xffff0000u)};
}
// the four bytes of w, each less `bias`, as bf16 (v_cvt_f32_ubyte0 .. 3)
__device__ __forceinline__ u32x2 ubytes4_to_bf16(uint32_t w, float bias)
{
    return ints4_to_bf16((float)(w & 0xffu) - bias, (float)((w >> 8) & 0xffu) - bias, (float)((w >> 16) & 0xffu) - bias, (float)(w >> 24) - bias);
}
__device__ __forceinline__ u32x2 sbytes4_to_bf16(uint32_t w)
{
    return ints4_to_bf16((float)(int8_t)(w & 0xffu), (float)(int8_t)((w >> 8) & 0xffu), (float)(int8_t)((w >> 16) & 0xffu), (float)(int8_t)(w >> 24));
}

// What a lane holds of one 32-wide K step of the weights: its eight codes as loaded (c; Q6_K: ql bytes in c, qh bytes in h) and the
// scales of its own output column for the step (Q8_0: s0 = d; Q4_K: s0 = d*sc_j, s1 = dmin*m_j; Q6_K: s0 / s1 = d * sc of the two
// 16-element sub-blocks).
struct GgStep {
    u32x2 c, h;
    float s0, s1;
};

// One workgroup per (64 x 64 tile, K slice): 256 threads, four waves of one 32 x 32 tile each, LDS double-buffered as
// [stage][A1 | A2 | A3 | W] with the stage's 64 activation row sums beside it (Q4_K).
template <uint32_t T, bool RESIDUAL>
__global__ __launch_bounds__(256) void prefill_gemm_ggmlw_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ Wq,
                                                                 const uint8_t* __restrict__ Wq2, const float* __restrict__ Ws,
                                                                 const int8_t* __restrict__ Ws2, const float* __restrict__ bias, const float* R,
                                                                 int64_t ldr, float* Y, int64_t ldy, int M, int N, int K, int m_tiles, int ksplit,
                                                                 float* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) uint16_t sp[2][4 * GG_PLANE];
    __shared__ __attribute__((aligned(16))) float srow[2][GG_BM];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    // the tile order of prefill_gemm_kernel: consecutive tiles on one XCD
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned bid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    const int ks = (int)(bid0 % (unsigned)ksplit);
    const unsigned bid = bid0 / (unsigned)ksplit;
    const int m0 = (int)(bid % (unsigned)m_tiles) * GG_BM;
    const int n0 = (int)(bid / (unsigned)m_tiles) * GG_BN;
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
    // the weight row this lane loads codes of (eight per K step) and the one it accumulates (its scales); past N: the last row again
    const int64_t w_row = min(n0 + b_row, N - 1), s_row = min(n0 + wc * 32 + l31, N - 1);
    const int nb = K >> 8;  // (K-quants) 256-blocks per row
    const int stW = 3 * GG_PLANE + b_row * 32 + (b_c ^ ((b_row >> 2) & 3)) * 8;
    f32x4 ga[2];
    GgStep gw;
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
        const int ka = k_begin + k0;  // absolute: the step's first column of K
        if (T == GGML_Q8_0) {
            gw.c = *reinterpret_cast<const u32x2*>(Wq + w_row * K + ka + b_c * 8);
            gw.s0 = Ws[s_row * (K >> 5) + (ka >> 5)];
        } else if (T == GGML_Q4_K) {
            const int blk = ka >> 8, sub = (ka >> 5) & 7;  // sub-block 2j + hi: chunk j = sub >> 1, its low (hi = 0) or high nibbles
            gw.c = *reinterpret_cast<const u32x2*>(Wq + (w_row * nb + blk) * 128 + (sub >> 1) * 32 + b_c * 8);
            const float* sc = Ws + (s_row * nb + blk) * 16 + sub;
            gw.s0 = sc[0];
            gw.s1 = sc[8];
        } else {
            const int blk = ka >> 8, hf = (ka >> 7) & 1, g = (ka >> 5) & 3;  // launch_qdequant's element order (q_element)
            gw.c = *reinterpret_cast<const u32x2*>(Wq + (w_row * nb + blk) * 128 + hf * 64 + (g & 1) * 32 + b_c * 8);
            gw.h = *reinterpret_cast<const u32x2*>(Wq2 + (w_row * nb + blk) * 64 + hf * 32 + b_c * 8);
            const float d = Ws[s_row * nb + blk];
            const uint32_t s2 = *reinterpret_cast<const uint16_t*>(Ws2 + (s_row * nb + blk) * 16 + hf * 8 + 2 * g);  // sub-blocks kk / 16 = 0, 1
            gw.s0 = d * (float)(int8_t)(s2 & 0xffu);
            gw.s1 = d * (float)(int8_t)(s2 >> 8);
        }
    };
    auto store = [&](int stage, int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p1, p2, p3;
            sp_split(ga[i], p1, p2, p3);
            *reinterpret_cast<u32x2*>(&sp[stage][stA[i]]) = p1;
            *reinterpret_cast<u32x2*>(&sp[stage][GG_PLANE + stA[i]]) = p2;
            *reinterpret_cast<u32x2*>(&sp[stage][2 * GG_PLANE + stA[i]]) = p3;
            if (T == GGML_Q4_K) {  // the row's sum over the step's 32 columns: the eight lanes a_c4 = 0 .. 7 of the row
                float rs = (ga[i][0] + ga[i][1]) + (ga[i][2] + ga[i][3]);
                rs += __shfl_xor(rs, 1, 64);
                rs += __shfl_xor(rs, 2, 64);
                rs += __shfl_xor(rs, 4, 64);
                if (a_c4 == 0) srow[stage][a_row + 32 * i] = rs;
            }
        }
        u32x2 o[2];  // the eight codes as bf16 integers: unpacked once per element, here
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (T == GGML_Q8_0) {
                o[d] = sbytes4_to_bf16(gw.c[d]);
            } else if (T == GGML_Q4_K) {
                const int sh = (((k_begin + k0) >> 5) & 1) * 4;  // odd sub-block: the high nibbles
                o[d] = ubytes4_to_bf16((gw.c[d] >> sh) & 0x0f0f0f0fu, 0.0f);
            } else {
                const int g = ((k_begin + k0) >> 5) & 3;  // nibble (g >> 1) of ql, bit pair g of qh
                o[d] = ubytes4_to_bf16(((gw.c[d] >> ((g >> 1) * 4)) & 0x0f0f0f0fu) | (((gw.h[d] >> (2 * g)) & 0x03030303u) << 4), 32.0f);
            }
        }
        *reinterpret_cast<u32x4*>(&sp[stage][stW]) = u32x4{o[0][0], o[0][1], o[1][0], o[1][1]};
    };
    f32x16 acc, total;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = total[r] = 0.0f;
    const int nk = k_len / GG_BK;
    const int fsw = (l31 >> 2) & 3;
    const int fa = (wr * 32 + l31) * 32, fb = 3 * GG_PLANE + (wc * 32 + l31) * 32;
    load(0);
    store(0, 0);
    float s0 = gw.s0, s1 = gw.s1;  // the scales of the step in LDS
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * GG_BK);  // codes and scales of the next step, in flight under this one's MFMAs
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int ch = ((kb * 2 + half) ^ fsw) * 8;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&sp[cur][fb + ch]);
#pragma unroll
            for (int p = 2; p >= 0; --p) {  // the smallest piece first
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sp[cur][p * GG_PLANE + fa + ch]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
            if (T == GGML_Q6_K) {  // a 16-element sub-block ends with each MFMA group
                const float s = kb ? s1 : s0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    total[r] += s * acc[r];
                    acc[r] = 0.0f;
                }
            }
        }
        if (T == GGML_Q8_0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                total[r] += s0 * acc[r];
                acc[r] = 0.0f;
            }
        } else if (T == GGML_Q4_K) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // accumulator rows 8g + 4 half .. + 3 (acc_row): one 16-byte read
                const f32x4 rs = *reinterpret_cast<const f32x4*>(&srow[cur][wr * 32 + 8 * g + 4 * half]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    total[4 * g + i] += s0 * acc[4 * g + i] - s1 * rs[i];
                    acc[4 * g + i] = 0.0f;
                }
            }
        }
        if (kt + 1 < nk) {
            store(cur ^ 1, (kt + 1) * GG_BK);
            s0 = gw.s0;
            s1 = gw.s1;
        }
        __syncthreads();
    }
    const int col = n0 + wc * 32 + l31;
    if (col < N) {
        if (ksplit > 1) {  // a finished partial (scales applied): prefill_splitk_reduce_kernel adds the slabs and the epilogue
            float* out = P + (int64_t)ks * M * N;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * 32 + acc_row(r, half);
                if (row < M) out[(int64_t)row * N + col] = total[r];
            }
            return;
        }
        const float bv = bias ? bias[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wr * 32 + acc_row(r, half);
            if (row < M) {
                float v = total[r] + bv;
                if (RESIDUAL) v += R[(int64_t)row * ldr + col];
                Y[(int64_t)row * ldy + col] = v;
            }
        }
    }
}

bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

hipError_t launch_prefill_gemm_ggml(const float* A, int64_t lda, const QMat& W, const float* bias, const float* R, int64_t ldr, float* Y,
                                    int64_t ldy, int M, hipStream_t stream, float* split_scratch, float* silu_gate)
{
    const int N = W.n, K = W.k;
    if (M <= 0 || N <= 0) return hipSuccess;
    if (!ggml_matrix_type(W.type)) return hipErrorInvalidValue;
    if (K <= 0 || K % (W.type == GGML_Q8_0 ? 32 : 256) || lda % 4 || off16(A)) return hipErrorInvalidValue;
    if (!W.q || !W.s || off16(W.q) || off16(W.s)) return hipErrorInvalidValue;
    if (W.type == GGML_Q6_K && (!W.q2 || !W.s2 || off16(W.q2) || off16(W.s2))) return hipErrorInvalidValue;
    if (silu_gate && (ldy != N || (N & 3) || off16(silu_gate))) return hipErrorInvalidValue;
    const int m_tiles = (M + GG_BM - 1) / GG_BM, n_tiles = (N + GG_BN - 1) / GG_BN;
    const int ksplit = prefill_gemm_launch_ksplit(bias, R, ldr, Y, ldy, M, N, K, split_scratch);  // (slices of a multiple of 32 columns)
    const dim3 grid((unsigned)(m_tiles * n_tiles * ksplit));
#define KJ_GG(TYPE, RES)                                                                                                                  \
    hipLaunchKernelGGL((prefill_gemm_ggmlw_kernel<TYPE, RES>), grid, dim3(256), 0, stream, A, lda, static_cast<const uint8_t*>(W.q),       \
                       static_cast<const uint8_t*>(W.q2), static_cast<const float*>(W.s), static_cast<const int8_t*>(W.s2), bias, R, ldr, Y, \
                       ldy, M, N, K, m_tiles, ksplit, split_scratch)
#define KJ_GG_TYPE(TYPE)           \
    do {                           \
        if (R) KJ_GG(TYPE, true);  \
        else KJ_GG(TYPE, false);   \
    } while (0)
    if (W.type == GGML_Q8_0) KJ_GG_TYPE(GGML_Q8_0);
    else if (W.type == GGML_Q4_K) KJ_GG_TYPE(GGML_Q4_K);
    else KJ_GG_TYPE(GGML_Q6_K);
#undef KJ_GG_TYPE
#undef KJ_GG
    if (ksplit > 1) return launch_prefill_splitk_reduce(split_scratch, ksplit, bias, R, ldr, Y, ldy, M, N, silu_gate, stream);
    if (silu_gate) return launch_swiglu_mul(silu_gate, Y, (size_t)M * N, stream);
    return hipGetLastError();
}

}  // namespace kjarni
