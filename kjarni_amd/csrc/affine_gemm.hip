// The prompt GEMM over the affine-32 planes (GGUF Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K as repack_affine32 leaves them; the layout is at
// the top of affine_kernels.hip) on the bf16 matrix cores: Y[M, N] = A . W^T with the nibbles and fifth bits read from HBM and
// unpacked into bf16 integer operands on the way into LDS -- no f32 or bf16 copy of the matrix through HBM (launch_affine_dequant +
// the f32 GEMM is the route this replaces where the decoder's switch is on).
//
// The tile shape, tile order over the XCDs, K slices, partial slabs, reduce kernel, LDS swizzle, MFMA loop and the three exact bf16
// activation planes are prefill_gemm_ggmlw_kernel's (ggml_gemm.hip).  This kernel's own:
//
// K step = one run of 32.  Byte i of a run's 16 holds element i (low nibble) and element i + 16 (high nibble), so the low nibbles
// of a run are exactly the first 16-wide MFMA K group of the step and the high nibbles the second.  Four lanes per weight row; a
// lane loads ONE dword of the run (bytes 4 b_c .. + 3), and for a 5-bit type the run's one fifth-bit word (the four lanes of a row
// read the same address), and has eight codes: elements 4 b_c .. + 3 (K group 0) and 16 + 4 b_c .. + 3 (K group 1) -- two 8-byte LDS
// stores, into half-chunks of the row that the MFMA side reads as it reads every other operand.
//
// Centred codes.  The operand is q - c, c = 8 (4 bits) or 16 (5 bits), free on the byte-to-float conversion; with w = a q + b the
// fold of a run is total += a * acc + b' * rowsum, b' = fmaf(a, c, b), rowsum the activation row summed over the run.  Centring
// halves the magnitude of the two terms that cancel.  For Q4_0 / Q5_0 b is -c a exactly, b' is exactly 0 and the term is not
// compiled (OFFSET = false): the fold is Q8_0's, 16 FMAs per step and no LDS read.  With OFFSET the row sums are formed in the A
// loader and kept as 64 floats beside the stage, as for Q4_K.
//
// (a, b) of the lane's own output column is one 8-byte load per step at the ABSOLUTE run index (a K slice begins on any multiple of
// 32), in flight with the codes a step ahead.
//
// Eight instances: (4 | 5 bits) x (offset | none) x (residual | none).  Compiled with -fno-slp-vectorize and without packed f32
// operations, as ggml_gemm.hip.
#include <hip/hip_runtime.h>

#include "affine_kernels.h"
#include "bf16_split.h"
#include "device_utils.h"
#include "gguf.h"
#include "llm_kernels.h"

namespace kjarni {

namespace {

constexpr int AG_BM = 64, AG_BN = 64, AG_BK = 32;
constexpr int AG_PLANE = 64 * 32;  // bf16 per plane: 64 rows x 64 bytes, the four 16-byte chunks of a row swizzled by (row >> 2) & 3

// The four bytes of w (each at most 31), less c, as four bf16 (two dwords): a small integer is the high half of its f32.
__device__ __forceinline__ u32x2 codes4_to_bf16(uint32_t w, float c)
{
    const float f0 = (float)(w & 0xffu) - c, f1 = (float)((w >> 8) & 0xffu) - c, f2 = (float)((w >> 16) & 0xffu) - c, f3 = (float)(w >> 24) - c;
    return u32x2{(__builtin_bit_cast(uint32_t, f0) >> 16) | (__builtin_bit_cast(uint32_t, f1) & 0xffff0000u),
                 (__builtin_bit_cast(uint32_t, f2) >> 16) | (__builtin_bit_cast(uint32_t, f3) & 0xffff0000u)};
}
// bits s .. s + 3 of h to bit 4 of bytes 0 .. 3 (the four shifted copies of the multiply do not overlap)
__device__ __forceinline__ uint32_t fifth4(uint32_t h, int s) { return ((((h >> s) & 15u) * 0x00204081u) & 0x01010101u) << 4; }

// What a lane holds of one run of the weights: its dword of nibbles, the run's fifth bits, (a, b) of its own output column.
struct AgStep {
    uint32_t c, h;
    float a, b;
};

// One workgroup per (64 x 64 tile, K slice): 256 threads, four waves of one 32 x 32 tile each, LDS double-buffered as
// [stage][A1 | A2 | A3 | W] with the stage's 64 activation row sums beside it (OFFSET).
template <int BITS, bool OFFSET, bool RESIDUAL>
__global__ __launch_bounds__(256) void prefill_gemm_affine_kernel(const float* __restrict__ A, int64_t lda, const uint8_t* __restrict__ Wq,
                                                                  const uint32_t* __restrict__ Wh, const float* __restrict__ Ws,
                                                                  const float* __restrict__ bias, const float* R, int64_t ldr, float* Y,
                                                                  int64_t ldy, int M, int N, int K, int m_tiles, int ksplit,
                                                                  float* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) uint16_t sp[2][4 * AG_PLANE];
    __shared__ __attribute__((aligned(16))) float srow[OFFSET ? 2 : 1][OFFSET ? AG_BM : 4];
    constexpr float kCentre = BITS == 4 ? 8.0f : 16.0f;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    // the tile order of prefill_gemm_kernel: consecutive tiles on one XCD
    const unsigned nwg = gridDim.x, xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const unsigned q8 = nwg >> 3, r8 = nwg & 7u;
    const unsigned bid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    const int ks = (int)(bid0 % (unsigned)ksplit);
    const unsigned bid = bid0 / (unsigned)ksplit;
    const int m0 = (int)(bid % (unsigned)m_tiles) * AG_BM;
    const int n0 = (int)(bid / (unsigned)m_tiles) * AG_BN;
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
    // the weight row this lane loads codes of (eight per run) and the one it accumulates (its scales); past N: the last row again
    const int64_t w_row = min(n0 + b_row, N - 1), s_row = min(n0 + wc * 32 + l31, N - 1);
    const int runs = K >> 5, run0 = k_begin >> 5;  // runs of a row; the slice's first
    const uint8_t* q_ptr = Wq + (w_row * runs + run0) * 16 + 4 * b_c;
    const uint32_t* h_ptr = Wh + (w_row * runs + run0);
    const float* s_ptr = Ws + (s_row * runs + run0) * 2;
    // elements 4 b_c .. + 3 of K group 0 and of K group 1: four-element group b_c of chunks 0 | 1 and of chunks 2 | 3 of the row
    const int wsw = (b_row >> 2) & 3;
    const int stW0 = 3 * AG_PLANE + b_row * 32 + (((b_c >> 1) ^ wsw) * 2 + (b_c & 1)) * 4;
    const int stW1 = 3 * AG_PLANE + b_row * 32 + (((2 + (b_c >> 1)) ^ wsw) * 2 + (b_c & 1)) * 4;
    f32x4 ga[2];
    AgStep gw;
    auto load = [&](int kt) {  // step kt of the slice: run run0 + kt of the row
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + kt * AG_BK);
        gw.c = *reinterpret_cast<const uint32_t*>(q_ptr + (int64_t)kt * 16);
        if (BITS == 5) gw.h = h_ptr[kt];
        const float2 ab = *reinterpret_cast<const float2*>(s_ptr + 2 * (int64_t)kt);
        gw.a = ab.x;
        gw.b = ab.y;
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p1, p2, p3;
            sp_split(ga[i], p1, p2, p3);
            *reinterpret_cast<u32x2*>(&sp[stage][stA[i]]) = p1;
            *reinterpret_cast<u32x2*>(&sp[stage][AG_PLANE + stA[i]]) = p2;
            *reinterpret_cast<u32x2*>(&sp[stage][2 * AG_PLANE + stA[i]]) = p3;
            if (OFFSET) {  // the row's sum over the run: the eight lanes a_c4 = 0 .. 7 of the row
                float rs = (ga[i][0] + ga[i][1]) + (ga[i][2] + ga[i][3]);
                rs += __shfl_xor(rs, 1, 64);
                rs += __shfl_xor(rs, 2, 64);
                rs += __shfl_xor(rs, 4, 64);
                if (a_c4 == 0) srow[stage][a_row + 32 * i] = rs;
            }
        }
        uint32_t lo = gw.c & 0x0f0f0f0fu, hi = (gw.c >> 4) & 0x0f0f0f0fu;
        if (BITS == 5) {
            lo |= fifth4(gw.h, 4 * b_c);
            hi |= fifth4(gw.h, 16 + 4 * b_c);
        }
        *reinterpret_cast<u32x2*>(&sp[stage][stW0]) = codes4_to_bf16(lo, kCentre);
        *reinterpret_cast<u32x2*>(&sp[stage][stW1]) = codes4_to_bf16(hi, kCentre);
    };
    f32x16 acc, total;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = total[r] = 0.0f;
    const int nk = k_len / AG_BK;
    const int fsw = (l31 >> 2) & 3;
    const int fa = (wr * 32 + l31) * 32, fb = 3 * AG_PLANE + (wc * 32 + l31) * 32;
    load(0);
    store(0);
    float sa = gw.a, sb = OFFSET ? fmaf(gw.a, kCentre, gw.b) : 0.0f;  // the scales of the step in LDS
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load(kt + 1);  // codes and scales of the next run, in flight under this one's MFMAs
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int ch = ((kb * 2 + half) ^ fsw) * 8;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&sp[cur][fb + ch]);
#pragma unroll
            for (int p = 2; p >= 0; --p) {  // the smallest piece first
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sp[cur][p * AG_PLANE + fa + ch]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
        }
        if (!OFFSET) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                total[r] += sa * acc[r];
                acc[r] = 0.0f;
            }
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // accumulator rows 8g + 4 half .. + 3 (acc_row): one 16-byte read
                const f32x4 rs = *reinterpret_cast<const f32x4*>(&srow[cur][wr * 32 + 8 * g + 4 * half]);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    total[4 * g + i] += sa * acc[4 * g + i] + sb * rs[i];
                    acc[4 * g + i] = 0.0f;
                }
            }
        }
        if (kt + 1 < nk) {
            store(cur ^ 1);
            sa = gw.a;
            if (OFFSET) sb = fmaf(gw.a, kCentre, gw.b);
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

hipError_t launch_prefill_gemm_affine(const float* A, int64_t lda, const QMat& W, const float* bias, const float* R, int64_t ldr, float* Y,
                                      int64_t ldy, int M, hipStream_t stream, float* split_scratch, float* silu_gate)
{
    const int N = W.n, K = W.k;
    if (M <= 0 || N <= 0) return hipSuccess;
    if (!ggml_affine_type(W.type)) return hipErrorInvalidValue;
    if (K <= 0 || K % (W.type == GGML_Q5_K ? 256 : 32) || lda % 4 || off16(A)) return hipErrorInvalidValue;
    if (!W.q || !W.s || off16(W.q) || off16(W.s)) return hipErrorInvalidValue;
    const int bits = affine_code_bits(W.type);
    if (bits == 5 && (!W.q2 || off16(W.q2))) return hipErrorInvalidValue;
    if (silu_gate && (ldy != N || (N & 3) || off16(silu_gate))) return hipErrorInvalidValue;
    const bool offset = !(W.type == GGML_Q4_0 || W.type == GGML_Q5_0);  // (d, -c d): b' = fmaf(d, c, -c d) is exactly 0
    const int m_tiles = (M + AG_BM - 1) / AG_BM, n_tiles = (N + AG_BN - 1) / AG_BN;
    const int ksplit = prefill_gemm_launch_ksplit(bias, R, ldr, Y, ldy, M, N, K, split_scratch);  // (slices of a multiple of 32 columns)
    const dim3 grid((unsigned)(m_tiles * n_tiles * ksplit));
#define KJ_AG(BITS, OFF, RES)                                                                                                              \
    hipLaunchKernelGGL((prefill_gemm_affine_kernel<BITS, OFF, RES>), grid, dim3(256), 0, stream, A, lda, static_cast<const uint8_t*>(W.q),  \
                       static_cast<const uint32_t*>(W.q2), static_cast<const float*>(W.s), bias, R, ldr, Y, ldy, M, N, K, m_tiles, ksplit, \
                       split_scratch)
#define KJ_AG_RES(BITS, OFF)            \
    do {                                \
        if (R) KJ_AG(BITS, OFF, true);  \
        else KJ_AG(BITS, OFF, false);   \
    } while (0)
    if (bits == 4 && !offset) KJ_AG_RES(4, false);
    else if (bits == 4) KJ_AG_RES(4, true);
    else if (!offset) KJ_AG_RES(5, false);
    else KJ_AG_RES(5, true);
#undef KJ_AG_RES
#undef KJ_AG
    if (ksplit > 1) return launch_prefill_splitk_reduce(split_scratch, ksplit, bias, R, ldr, Y, ldy, M, N, silu_gate, stream);
    if (silu_gate) return launch_swiglu_mul(silu_gate, Y, (size_t)M * N, stream);
    return hipGetLastError();
}

}  // namespace kjarni
