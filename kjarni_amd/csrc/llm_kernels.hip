// Kernels of the decoder-only (Llama / Qwen2 / GPT-2) path: a weight-streaming GEMV for 1-8 rows over f32 or bf16
// weights with RMSNorm or LayerNorm folded in and the Q|K|V, SwiGLU, GELU-tanh and residual epilogues; RoPE; embedding
// gather (with learned positions for GPT-2); a two-stage argmax.  Attention over the KV cache reuses decode_attention_* (whisper_kernels.hip) with a
// grouped-query head mapping.
//
//   RMSNorm   crates/kjarni-transformers/src/cpu/normalization/rms_norm.rs:19-27
//   RoPE      cpu/rope/mod.rs:107-176
//   layer     cpu/decoder/rope_decoder_layer.rs:18-41, cpu/decoder/decoder_attention.rs:44-170,
//             cpu/feedforward/swiglu.rs:32-57
//   greedy    common/sampling.rs:83-88
#include <algorithm>

#include "device_utils.h"
#include "dynamic_lds.h"
#include "llm_kernels.h"
#include "kernels.h"

namespace kjarni {

namespace {

constexpr int LLM_MAX_ROWS = 8;

struct F8 {
    float v[8];
};

// Eight consecutive weights starting at element 8*i of a row.
__device__ __forceinline__ F8 load8(const float* row, int i)
{
    const f32x4 a = *reinterpret_cast<const f32x4*>(row + i * 8);
    const f32x4 b = *reinterpret_cast<const f32x4*>(row + i * 8 + 4);
    return F8{{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
}
__device__ __forceinline__ F8 load8(const uint16_t* row, int i)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 p = *reinterpret_cast<const u32x4*>(row + i * 8);
    F8 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        r.v[2 * c] = __uint_as_float(p[c] << 16);
        r.v[2 * c + 1] = __uint_as_float(p[c] & 0xFFFF0000u);
    }
    return r;
}

enum : int { LE_NONE = 0, LE_RESIDUAL = 1, LE_SWIGLU = 2, LE_GELU_TANH = 3 };
// Row normalisation in a kernel's prologue: none, RMSNorm (Llama) or LayerNorm with a bias (GPT-2: (x - mean) / sqrt(var + eps)
// * gamma + beta, the arithmetic of the encoder's layernorm kernels, rowops.hip).
enum : int { NK_NONE = 0, NK_RMS = 1, NK_LN = 2 };

// Y[r, n] = epi(norm?(X[r, :]) . W[n, :] + bias[n]) for up to 8 rows; one wave per output column.
//  NORM: rows are RMS-normalised on the fly: (x / sqrt(mean(x^2) + eps)) * gamma, statistics recomputed per wave
//  (NK_LN: LayerNorm, mean and variance in two passes, + beta).
//  LE_GELU_TANH: gelu_tanh(x.W[n] + bias[n]).
//  LE_SWIGLU: W2 is the `up` matrix; the output is silu(x.W[n]) * (x.W2[n]).
//  LE_RESIDUAL: + R[r, n].
//  seg > 0: columns [0,seg_q) -> Y0, then two segments of seg_kv columns -> Y1 / Y2 at row (*row_off_ptr | row_off) + r
//  (Q to scratch, K and V straight into the cache).
template <typename WT, int EPI, int NORM>
__global__ __launch_bounds__(256) void llm_gemv_kernel(const float* __restrict__ X, int64_t ldx, int rows,
                                                       const float* __restrict__ gamma, float eps, const WT* __restrict__ W,
                                                       const WT* __restrict__ W2, const float* __restrict__ bias,
                                                       const float* __restrict__ R, int64_t ldr, int n_out, int k, int seg_q,
                                                       int seg_kv, float* __restrict__ Y0, int64_t ldy0, float* __restrict__ Y1,
                                                       float* __restrict__ Y2, int64_t ldy12, int row_off,
                                                       const int* __restrict__ row_off_ptr, const float* __restrict__ beta)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_out) return;
    const int k8 = k >> 3;
    float scale[LLM_MAX_ROWS], mu[LLM_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < LLM_MAX_ROWS; ++r) scale[r] = 1.0f, mu[r] = 0.0f;
    if (NORM == NK_LN) {
#pragma unroll
        for (int r = 0; r < LLM_MAX_ROWS; ++r) {
            if (r < rows) {
                float s = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(X + r * ldx, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) s += x.v[c];
                }
                const float m = wave_sum(s) / (float)k;
                float v = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(X + r * ldx, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) v = fmaf(x.v[c] - m, x.v[c] - m, v);
                }
                mu[r] = m;
                scale[r] = 1.0f / sqrtf(wave_sum(v) / (float)k + eps);  // the inverse standard deviation
            }
        }
    }
    if (NORM == NK_RMS) {
#pragma unroll
        for (int r = 0; r < LLM_MAX_ROWS; ++r) {
            if (r < rows) {
                float s = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(X + r * ldx, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) s = fmaf(x.v[c], x.v[c], s);
                }
                scale[r] = sqrtf(wave_sum(s) / (float)k + eps);  // the rms; the reference divides by it
            }
        }
    }
    const WT* w_row = W + n * (int64_t)k;
    const WT* w2_row = EPI == LE_SWIGLU ? W2 + n * (int64_t)k : nullptr;
    float acc[LLM_MAX_ROWS], acc2[LLM_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < LLM_MAX_ROWS; ++r) acc[r] = acc2[r] = 0.0f;
    for (int i = lane; i < k8; i += 64) {
        const F8 w = load8(w_row, i);
        F8 w2;
        if (EPI == LE_SWIGLU) w2 = load8(w2_row, i);
        F8 g, be;
        if (NORM) g = load8(gamma, i);
        if (NORM == NK_LN) be = load8(beta, i);
#pragma unroll
        for (int r = 0; r < LLM_MAX_ROWS; ++r) {
            if (r < rows) {
                F8 x = load8(X + r * ldx, i);
                if (NORM == NK_RMS) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) x.v[c] = (x.v[c] / scale[r]) * g.v[c];
                }
                if (NORM == NK_LN) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) x.v[c] = (x.v[c] - mu[r]) * scale[r] * g.v[c] + be.v[c];
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    acc[r] = fmaf(x.v[c], w.v[c], acc[r]);
                    if (EPI == LE_SWIGLU) acc2[r] = fmaf(x.v[c], w2.v[c], acc2[r]);
                }
            }
        }
    }
    const float b = bias ? bias[n] : 0.0f;
    int which = 0;
    int64_t col = n;
    if (seg_q > 0 && n >= seg_q) {
        which = 1 + (int)((n - seg_q) / seg_kv);
        col = (n - seg_q) - (int64_t)(which - 1) * seg_kv;
    }
    float* Y = which == 0 ? Y0 : (which == 1 ? Y1 : Y2);
    const int64_t ldy = which == 0 ? ldy0 : ldy12;
    const int64_t r0 = which == 0 ? 0 : (row_off_ptr ? *row_off_ptr : row_off);
#pragma unroll
    for (int r = 0; r < LLM_MAX_ROWS; ++r) {
        if (r < rows) {
            float v = wave_sum(acc[r]) + b;
            if (EPI == LE_SWIGLU) {
                const float u = wave_sum(acc2[r]);
                v = (v / (1.0f + expf(-v))) * u;  // silu(gate) * up
            }
            if (EPI == LE_GELU_TANH) v = gelu_tanh(v);
            if (EPI == LE_RESIDUAL) v += R[r * ldr + n];
            if (lane == 0) Y[(r0 + r) * ldy + col] = v;
        }
    }
}

// Single-row variant (the decode step).  The input row is normalised once per WORKGROUP into LDS (the
// multi-row kernel re-reads it from L2 for every output column, which costs more L2 bandwidth than the bf16
// weights cost HBM bandwidth); each wave then streams OPW weight rows, with all of a row's 16-byte loads in
// flight before the first FMA.
constexpr int G1_OPW = 2;        // outputs per wave
constexpr int G1_MAX_K = 16384;  // 64 KiB of LDS

template <typename WT, int EPI, int NORM>
__global__ __launch_bounds__(256) void llm_gemv1_kernel(const float* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                        const WT* __restrict__ W, const WT* __restrict__ W2,
                                                        const float* __restrict__ bias, const float* __restrict__ R, int n_out,
                                                        int k, int seg_q, int seg_kv, float* __restrict__ Y0,
                                                        float* __restrict__ Y1, float* __restrict__ Y2, int64_t ldy12, int row_off,
                                                        const int* __restrict__ row_off_ptr, const float* __restrict__ beta)
{
    extern __shared__ float xs[];  // [k]
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k8 = k >> 3;
    float rms = 1.0f, mu = 0.0f, inv = 1.0f;
    if (NORM == NK_LN) {  // mean, then the variance around it: two passes over the row (L2-resident)
        float s = 0.0f;
        for (int i = tid; i < k8; i += 256) {
            const F8 x = load8(X, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) s += x.v[c];
        }
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        mu = ((red[0] + red[1]) + (red[2] + red[3])) / (float)k;
        __syncthreads();
        float v = 0.0f;
        for (int i = tid; i < k8; i += 256) {
            const F8 x = load8(X, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) v = fmaf(x.v[c] - mu, x.v[c] - mu, v);
        }
        v = wave_sum(v);
        if (lane == 0) red[wave] = v;
        __syncthreads();
        inv = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)k + eps);
    }
    if (NORM == NK_RMS) {
        float s = 0.0f;
        for (int i = tid; i < k8; i += 256) {
            const F8 x = load8(X, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) s = fmaf(x.v[c], x.v[c], s);
        }
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)k + eps);
    }
    for (int i = tid; i < k8; i += 256) {
        F8 x = load8(X, i);
        if (NORM == NK_RMS) {
            const F8 g = load8(gamma, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) x.v[c] = (x.v[c] / rms) * g.v[c];
        }
        if (NORM == NK_LN) {
            const F8 g = load8(gamma, i), be = load8(beta, i);
#pragma unroll
            for (int c = 0; c < 8; ++c) x.v[c] = (x.v[c] - mu) * inv * g.v[c] + be.v[c];
        }
        *reinterpret_cast<f32x4*>(xs + i * 8) = f32x4{x.v[0], x.v[1], x.v[2], x.v[3]};
        *reinterpret_cast<f32x4*>(xs + i * 8 + 4) = f32x4{x.v[4], x.v[5], x.v[6], x.v[7]};
    }
    __syncthreads();

    const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * G1_OPW;
#pragma unroll
    for (int j = 0; j < G1_OPW; ++j) {
        const int64_t n = n0 + j;
        if (n >= n_out) break;
        const WT* w_row = W + n * (int64_t)k;
        const WT* w2_row = EPI == LE_SWIGLU ? W2 + n * (int64_t)k : nullptr;
        float acc = 0.0f, acc2 = 0.0f;
        for (int i0 = lane; i0 < k8; i0 += 256) {  // four chunks per lane per trip: 4 (8 with SwiGLU) loads in flight
            F8 w[4], u[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q * 64;
                if (i < k8) {
                    w[q] = load8(w_row, i);
                    if (EPI == LE_SWIGLU) u[q] = load8(w2_row, i);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q * 64;
                if (i < k8) {
                    const f32x4 xa = *reinterpret_cast<const f32x4*>(xs + i * 8);
                    const f32x4 xb = *reinterpret_cast<const f32x4*>(xs + i * 8 + 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc = fmaf(xa[c], w[q].v[c], acc);
                        acc = fmaf(xb[c], w[q].v[4 + c], acc);
                        if (EPI == LE_SWIGLU) {
                            acc2 = fmaf(xa[c], u[q].v[c], acc2);
                            acc2 = fmaf(xb[c], u[q].v[4 + c], acc2);
                        }
                    }
                }
            }
        }
        float v = wave_sum(acc) + (bias ? bias[n] : 0.0f);
        if (EPI == LE_SWIGLU) {
            const float up = wave_sum(acc2);
            v = (v / (1.0f + expf(-v))) * up;
        }
        if (EPI == LE_RESIDUAL) v += R[n];
        if (lane == 0) {
            int which = 0;
            int64_t col = n;
            if (seg_q > 0 && n >= seg_q) {
                which = 1 + (int)((n - seg_q) / seg_kv);
                col = (n - seg_q) - (int64_t)(which - 1) * seg_kv;
            }
            float* Y = which == 0 ? Y0 : (which == 1 ? Y1 : Y2);
            const int64_t r0 = which == 0 ? 0 : (row_off_ptr ? *row_off_ptr : row_off);
            Y[which == 0 ? col : r0 * ldy12 + col] = v;
        }
    }
}

// Single-row GEMV with the K dimension split over the four waves of a workgroup.  A workgroup owns SK_OPW output
// columns; lane t of the block keeps chunks t, t+256, ... of the input row in registers (normalised in place when
// NORM — the sum of squares is reduced once through LDS), issues every weight load of its slice before the first
// FMA (SK_OPW x chunks x 16 bytes per lane in flight) and the four per-wave partial sums meet in LDS.  Compared with
// one wave per column this puts 4x more workgroups on the chip for the narrow projections (o, down) and reads the
// input row once per SK_OPW columns instead of once per column.
constexpr int SK_MAX_CHUNKS = 8;  // k <= 8 * 256 * 8 = 16384 with 4 waves; long rows (k >= 8192) use 16 waves per workgroup
// Two columns per workgroup measured best on every projection of the 1B and 8B shapes (1, 4 and 8 were 2-18 % slower end
// to end): the chip wants many small workgroups more than it wants deep per-lane load queues.
constexpr int SK_OPW = 2;

template <typename WT, int EPI, int NORM, int CH, int NW>
__global__ __launch_bounds__(64 * NW) void llm_gemv_splitk_kernel(const float* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                              const WT* __restrict__ W, const WT* __restrict__ W2,
                                                              const float* __restrict__ bias, const float* __restrict__ R,
                                                              int n_out, int k, float* __restrict__ Y, const float* __restrict__ beta)
{
    constexpr int NM = EPI == LE_SWIGLU ? 2 : 1;
    constexpr int THREADS = 64 * NW;
    __shared__ float red[NW];
    __shared__ float part[NW][NM * SK_OPW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k8 = k >> 3;
    F8 x[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int i = tid + c * THREADS;
        if (i < k8) x[c] = load8(X, i);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[c].v[e] = 0.0f;
        }
    }
    const int64_t n0 = (int64_t)blockIdx.x * SK_OPW;
    // Weight loads do not depend on the statistics: issue them first so the reduction overlaps their latency.
    F8 w[SK_OPW][CH], u[EPI == LE_SWIGLU ? SK_OPW : 1][CH];
#pragma unroll
    for (int o = 0; o < SK_OPW; ++o) {
        const int64_t n = n0 + o < n_out ? n0 + o : n_out - 1;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * THREADS;
            if (i < k8) {
                w[o][c] = load8(W + n * (int64_t)k, i);
                if (EPI == LE_SWIGLU) u[o][c] = load8(W2 + n * (int64_t)k, i);
            }
        }
    }
    if (NORM == NK_LN) {  // mean (the zero padding adds nothing), then the variance around it over the row's own chunks
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += x[c].v[e];
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float total = 0.0f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) total += red[wv];
        const float mean = total / (float)k;
        __syncthreads();
        float v = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            if (tid + c * THREADS < k8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v = fmaf(x[c].v[e] - mean, x[c].v[e] - mean, v);
            }
        v = wave_sum(v);
        if (lane == 0) red[wave] = v;
        __syncthreads();
        float vt = 0.0f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) vt += red[wv];
        const float inv = 1.0f / sqrtf(vt / (float)k + eps);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * THREADS;
            if (i < k8) {
                const F8 g = load8(gamma, i), be = load8(beta, i);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[c].v[e] = (x[c].v[e] - mean) * inv * g.v[e] + be.v[e];
            }
        }
    }
    if (NORM == NK_RMS) {
        float s = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) s = fmaf(x[c].v[e], x[c].v[e], s);
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        float total = 0.0f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) total += red[wv];
        const float rms = sqrtf(total / (float)k + eps);
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * THREADS;
            if (i < k8) {
                const F8 g = load8(gamma, i);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[c].v[e] = (x[c].v[e] / rms) * g.v[e];
            }
        }
    }
#pragma unroll
    for (int o = 0; o < SK_OPW; ++o) {
        float acc = 0.0f, acc2 = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * THREADS;
            if (i < k8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    acc = fmaf(x[c].v[e], w[o][c].v[e], acc);
                    if (EPI == LE_SWIGLU) acc2 = fmaf(x[c].v[e], u[o][c].v[e], acc2);
                }
            }
        }
        acc = wave_sum(acc);
        if (EPI == LE_SWIGLU) acc2 = wave_sum(acc2);
        if (lane == 0) {
            part[wave][o] = acc;
            if (EPI == LE_SWIGLU) part[wave][SK_OPW + o] = acc2;
        }
    }
    __syncthreads();
    if (tid < SK_OPW && n0 + tid < n_out) {
        const int64_t n = n0 + tid;
        float v = 0.0f;
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) v += part[wv][tid];
        v += bias ? bias[n] : 0.0f;
        if (EPI == LE_SWIGLU) {
            float up = 0.0f;
#pragma unroll
            for (int wv = 0; wv < NW; ++wv) up += part[wv][SK_OPW + tid];
            v = (v / (1.0f + expf(-v))) * up;
        }
        if (EPI == LE_GELU_TANH) v = gelu_tanh(v);
        if (EPI == LE_RESIDUAL) v += R[n];
        Y[n] = v;
    }
}

// Single-row GEMV as a weight STREAM (rows == 1, bf16 or f32 weights, K = 64 lanes x 8 elements x CH pieces): what a
// decode step is made of is reading every weight once, so the kernel is built around keeping 16-byte loads in flight.
// A few long-lived workgroups instead of thousands of two-column ones: the input row is normalised ONCE per workgroup
// into LDS, then every wave walks whole weight rows -- a batch is RB rows x CH pieces = 16 (32 with the SwiGLU pair)
// non-temporal 16-byte loads per lane, all issued before the first FMA (the weights are read once: nt keeps them
// from evicting what the other kernels of the step re-read) -- multiplies them with its LDS-resident slice of x and
// finishes each row with a wave reduction.  Rows are dealt batch by batch over all waves of the grid.
template <int N>
struct RawPieces {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v[N];
};

__device__ __forceinline__ RawPieces<1>::u32x4 load_nt16(const void* p)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}

// dot of 8 consecutive weights (one 16-byte bf16 piece, or the pair of f32 pieces p0 / p1) with x[0..7]
__device__ __forceinline__ float dot8_bf16(RawPieces<1>::u32x4 p, const f32x4 xa, const f32x4 xb, float acc)
{
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float lo = __uint_as_float(p[c] << 16), hi = __uint_as_float(p[c] & 0xFFFF0000u);
        const float x0 = c < 2 ? xa[2 * c] : xb[2 * c - 4], x1 = c < 2 ? xa[2 * c + 1] : xb[2 * c - 3];
        acc = fmaf(x0, lo, acc);
        acc = fmaf(x1, hi, acc);
    }
    return acc;
}

constexpr int stream_rows_per_batch(int ch, int loads_per_piece, int nm, bool wide)
{
    return wide && 16 / (ch * loads_per_piece * nm) > 1 ? 16 / (ch * loads_per_piece * nm) : 1;
}

template <typename WT, int EPI, bool NORM, int CH, bool WIDE, bool LOOP, int THREADS, int ATT = 0>
__global__ __launch_bounds__(THREADS) void llm_gemv_stream_kernel(const float* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                              const WT* __restrict__ W, const WT* __restrict__ W2,
                                                              const float* __restrict__ bias, const float* __restrict__ R,
                                                              int n_out, float* __restrict__ Y, int att_splits, int att_head_dim,
                                                              float* __restrict__ Xn)
{
    constexpr bool BF16 = sizeof(WT) == 2;
    constexpr int K = CH * 512;
    constexpr int NM = EPI == LE_SWIGLU ? 2 : 1;
    constexpr int LOADS_PER_PIECE = BF16 ? 1 : 2;                                // 8 weights = 16 or 32 bytes
    // rows per wave and batch: WIDE = 16 loads per lane in flight (large projections), else one row (a 2048-row projection
    // then still gives every CU 8 waves); LOOP = the grid does not cover the rows (the vocabulary head), else one batch per wave
    constexpr int RB = stream_rows_per_batch(CH, LOADS_PER_PIECE, NM, WIDE);
    __shared__ __attribute__((aligned(16))) float xs[K];
    constexpr int WAVES = THREADS / 64;  // 4 or 8: the larger workgroup halves the re-reads of the input row
    __shared__ float red[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: row bases stay in SGPRs
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int XV = K / (4 * THREADS);  // f32x4 pieces of the input row per thread
    // Everything the workgroup reads is requested before anything is waited for: the input row (and gamma), then the first
    // batch of weight rows.  The row is then normalised once per workgroup into LDS (x / sqrt(mean(x^2) + eps)) * gamma
    // (rms_norm.rs:19-27) while the weights are still in flight; the counter waits are in issue order, so x must go first.
    // ATT > 0: the row is the context row of the decode attention, still in ATT-or-fewer slabs per head (max, sum of exp,
    // sum of exp * V: whisper_kernels.hip); their merge (the arithmetic of decode_attention_combine_kernel) happens here,
    // under the weight requests, instead of in a launch of its own.
    constexpr int AS = ATT > 0 ? ATT : 1;
    f32x4 xv[XV], gv[XV], hv[XV][AS], av[XV][AS];
    if (ATT > 0) {
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int col = (tid + i * THREADS) * 4, head = col / att_head_dim, j = col - head * att_head_dim;
            const float* slab = X + (int64_t)head * att_splits * (att_head_dim + 4);
#pragma unroll
            for (int sp = 0; sp < AS; ++sp) {
                const float* p = slab + (sp < att_splits ? sp : 0) * (att_head_dim + 4);
                hv[i][sp] = *reinterpret_cast<const f32x4*>(p);
                av[i][sp] = *reinterpret_cast<const f32x4*>(p + 4 + j);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < XV; ++i) xv[i] = *reinterpret_cast<const f32x4*>(X + (tid + i * THREADS) * 4);
    }
    if (NORM) {
#pragma unroll
        for (int i = 0; i < XV; ++i) gv[i] = *reinterpret_cast<const f32x4*>(gamma + (tid + i * THREADS) * 4);
    }
    const int waves_total = gridDim.x * WAVES;
    u32x4 raw[NM][RB][CH][LOADS_PER_PIECE];
    auto issue = [&](int n0) {
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int n = n0 + r < n_out ? n0 + r : n_out - 1;
                const char* row = reinterpret_cast<const char*>((m == 0 ? W : W2) + (int64_t)n * K);
#pragma unroll
                for (int c = 0; c < CH; ++c)
#pragma unroll
                    for (int l = 0; l < LOADS_PER_PIECE; ++l)
                        raw[m][r][c][l] = load_nt16(row + ((size_t)(c * 64 + lane) * 8) * sizeof(WT) + l * 16);
            }
    };
    const int first = (blockIdx.x * WAVES + wave) * RB;
    float bv[RB], rv[RB];  // the epilogue's bias / residual values, requested ahead of the batch's weights
    auto issue_tail = [&](int n0) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int n = n0 + r < n_out ? n0 + r : n_out - 1;
            bv[r] = bias ? bias[n] : 0.0f;
            rv[r] = EPI == LE_RESIDUAL ? R[n] : 0.0f;
        }
    };
    issue_tail(first);
    issue(first);  // unconditional (rows past the end clamp to the last one): a branch here would make the x wait drain the weights too
    if (ATT > 0) {
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            float M = -INFINITY;
#pragma unroll
            for (int sp = 0; sp < AS; ++sp)
                if (sp < att_splits) M = fmaxf(M, hv[i][sp][0]);
            float L = 0.0f;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sp = 0; sp < AS; ++sp) {
                if (sp < att_splits) {
                    const float w = (hv[i][sp][0] == -INFINITY) ? 0.0f : expf(hv[i][sp][0] - M);
                    L = fmaf(hv[i][sp][1], w, L);
#pragma unroll
                    for (int c = 0; c < 4; ++c) a[c] = fmaf(av[i][sp][c], w, a[c]);
                }
            }
            const float inv = L > 0.0f ? 1.0f / L : 1.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) xv[i][c] = L > 0.0f ? a[c] * inv : a[c];
        }
    }
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < XV; ++i) ss += (xv[i][0] * xv[i][0] + xv[i][1] * xv[i][1]) + (xv[i][2] * xv[i][2] + xv[i][3] * xv[i][3]);
    if (NORM) {
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        float tot = (red[0] + red[1]) + (red[2] + red[3]);
        if (WAVES == 8) tot += (red[4] + red[5]) + (red[6] + red[7]);
        const float rms = sqrtf(tot / (float)K + eps);
#pragma unroll
        for (int i = 0; i < XV; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) xv[i][c] = (xv[i][c] / rms) * gv[i][c];
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) *reinterpret_cast<f32x4*>(xs + (tid + i * THREADS) * 4) = xv[i];
    if (NORM && Xn && blockIdx.x == 0) {  // the normalised row is an output too (the model's last hidden state)
#pragma unroll
        for (int i = 0; i < XV; ++i) *reinterpret_cast<f32x4*>(Xn + (tid + i * THREADS) * 4) = xv[i];
    }
    __syncthreads();

    // Per batch of RB rows: the NEXT batch's bias / residual values and weights are requested before this batch's cross-lane
    // sums and stores, which need no loads, so nothing ever waits with fresh requests behind it (the counter retires in
    // issue order, and the tail values, older than their batch's weights, have landed once the products are done).
    for (int n0 = first;;) {
        float acc[NM][RB];
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int r = 0; r < RB; ++r) acc[m][r] = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const f32x4 xa = *reinterpret_cast<const f32x4*>(xs + (c * 64 + lane) * 8);
            const f32x4 xb = *reinterpret_cast<const f32x4*>(xs + (c * 64 + lane) * 8 + 4);
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    if (BF16) {
                        acc[m][r] = dot8_bf16(raw[m][r][c][0], xa, xb, acc[m][r]);
                    } else {
                        const f32x4 wa = __builtin_bit_cast(f32x4, raw[m][r][c][0]);
                        const f32x4 wb = __builtin_bit_cast(f32x4, raw[m][r][c][LOADS_PER_PIECE - 1]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[m][r] = fmaf(xa[e], wa[e], acc[m][r]);
                            acc[m][r] = fmaf(xb[e], wb[e], acc[m][r]);
                        }
                    }
                }
        }
        float cb[RB], cr[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            cb[r] = bv[r];
            cr[r] = rv[r];
        }
        const int next = n0 + waves_total * RB;
        const bool more = LOOP && next < n_out;
        if (LOOP && more) {
            issue_tail(next);
            issue(next);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            float v = wave_sum(acc[0][r]);
            float up = 0.0f;
            if (EPI == LE_SWIGLU) up = wave_sum(acc[NM - 1][r]);
            const int n = n0 + r;
            if (lane == 0 && n < n_out) {
                v += cb[r];
                if (EPI == LE_SWIGLU) v = (v / (1.0f + expf(-v))) * up;
                if (EPI == LE_RESIDUAL) v += cr[r];
                Y[n] = v;
            }
        }
        if (!more) break;
        n0 = next;
    }
}

// Decode-step fusion of RMSNorm + Q|K|V projection + RoPE (decoder_attention.rs:61-97 for one new token).  Same split-K
// layout as llm_gemv_splitk_kernel (the four waves of a workgroup share the K dimension, the row is normalised in
// registers); a workgroup owns the PAIR of output columns (i, i + d/2) of one head, so it rotates its own two outputs
// (rope/mod.rs:156-176) before Q goes to scratch and K to its cache row; V columns go in pairs of neighbours, unrotated.
template <typename WT, int CH>
__global__ __launch_bounds__(256) void llm_qkv_rope_kernel(const float* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                           const WT* __restrict__ W, const float* __restrict__ bias, int k,
                                                           int n_heads, int n_kv_heads, int head_dim, const float* __restrict__ cos_t,
                                                           const float* __restrict__ sin_t, float* __restrict__ Q,
                                                           float* __restrict__ Kc, float* __restrict__ Vc, int pos,
                                                           const int* __restrict__ pos_ptr)
{
    __shared__ float red[4];
    __shared__ float part[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k8 = k >> 3, half = head_dim >> 1;
    const int q_dim = n_heads * head_dim, kv_dim = n_kv_heads * head_dim;
    const int q_tasks = q_dim / 2, k_tasks = kv_dim / 2;
    const int task = blockIdx.x;
    int n_a, n_b;  // the two output columns (rows of W) of this workgroup
    int kind;      // 0 = Q, 1 = K, 2 = V
    if (task < q_tasks + k_tasks) {
        kind = task < q_tasks ? 0 : 1;
        const int t = kind == 0 ? task : task - q_tasks;
        const int head = t / half, i = t - head * half;
        n_a = (kind == 0 ? 0 : q_dim) + head * head_dim + i;
        n_b = n_a + half;
    } else {
        kind = 2;
        n_a = q_dim + kv_dim + 2 * (task - q_tasks - k_tasks);
        n_b = n_a + 1;
    }
    F8 x[CH], wa[CH], wb[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int i = tid + c * 256;
        if (i < k8) {
            x[c] = load8(X, i);
            wa[c] = load8(W + (int64_t)n_a * k, i);
            wb[c] = load8(W + (int64_t)n_b * k, i);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) x[c].v[e] = wa[c].v[e] = wb[c].v[e] = 0.0f;
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(x[c].v[e], x[c].v[e], s);
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)k + eps);
    float acc_a = 0.0f, acc_b = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int i = tid + c * 256;
        if (i < k8) {
            const F8 g = load8(gamma, i);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xn = (x[c].v[e] / rms) * g.v[e];
                acc_a = fmaf(xn, wa[c].v[e], acc_a);
                acc_b = fmaf(xn, wb[c].v[e], acc_b);
            }
        }
    }
    acc_a = wave_sum(acc_a);
    acc_b = wave_sum(acc_b);
    if (lane == 0) {
        part[wave][0] = acc_a;
        part[wave][1] = acc_b;
    }
    __syncthreads();
    if (tid != 0) return;
    const float va = ((part[0][0] + part[1][0]) + (part[2][0] + part[3][0])) + (bias ? bias[n_a] : 0.0f);
    const float vb = ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1])) + (bias ? bias[n_b] : 0.0f);
    const int p = pos_ptr ? *pos_ptr : pos;
    if (kind == 2) {
        const int col = n_a - q_dim - kv_dim;
        Vc[(int64_t)p * kv_dim + col] = va;
        Vc[(int64_t)p * kv_dim + col + 1] = vb;
        return;
    }
    const int col = kind == 0 ? n_a : n_a - q_dim;
    const int i = col % head_dim;  // < half
    const float c = cos_t[(int64_t)p * half + i], sn = sin_t[(int64_t)p * half + i];
    float* out = kind == 0 ? Q : Kc + (int64_t)p * kv_dim;
    out[col] = va * c - vb * sn;
    out[col + half] = va * sn + vb * c;
}

// The same step in the weight-streaming form (K = 2048 / 4096 / 8192): one WAVE owns the pair of output columns, the row is
// normalised once per workgroup into LDS, and every request (x, gamma, position, the pair's two weight rows, bias, the
// rotation's cos / sin) is issued before anything is waited for.
// EMBED (the first layer of a one-token step): the input row is not read from X but gathered here from the embedding table, as
// llm_embed_kernel does (row *embed_ids, widened; an id >= vocab leaves zeros), by every workgroup for itself; workgroup 0 also
// stores it to x_raw_out, the residual stream the output projection adds to.  One launch fewer per token.
template <typename WT, int CH, bool EMBED = false>
__global__ __launch_bounds__(256) void llm_qkv_rope_stream_kernel(const float* __restrict__ X, const float* __restrict__ gamma, float eps,
                                                                  const WT* __restrict__ W, const float* __restrict__ bias,
                                                                  int n_heads, int n_kv_heads, int head_dim,
                                                                  const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                  float* __restrict__ Q, float* __restrict__ Kc, float* __restrict__ Vc,
                                                                  int pos, const int* __restrict__ pos_ptr,
                                                                  const uint32_t* __restrict__ embed_ids, const WT* __restrict__ table,
                                                                  int vocab, float* __restrict__ x_raw_out)
{
    constexpr bool BF16 = sizeof(WT) == 2;
    constexpr int K = CH * 512;
    constexpr int LOADS_PER_PIECE = BF16 ? 1 : 2;
    constexpr int XV = K / 1024;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float xs[K];
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = head_dim >> 1;
    const int q_dim = n_heads * head_dim, kv_dim = n_kv_heads * head_dim;
    const int q_tasks = q_dim / 2, k_tasks = kv_dim / 2, tasks = q_tasks + 2 * k_tasks;
    const int my = blockIdx.x * 4 + wave;
    const int task = my < tasks ? my : tasks - 1;  // surplus waves redo the last pair and store nothing
    int n_a, n_b, kind;  // the two output columns (rows of W) of this wave; 0 = Q, 1 = K, 2 = V
    if (task < q_tasks + k_tasks) {
        kind = task < q_tasks ? 0 : 1;
        const int t = kind == 0 ? task : task - q_tasks;
        const int head = t / half, i = t - head * half;
        n_a = (kind == 0 ? 0 : q_dim) + head * head_dim + i;
        n_b = n_a + half;
    } else {
        kind = 2;
        n_a = q_dim + kv_dim + 2 * (task - q_tasks - k_tasks);
        n_b = n_a + 1;
    }
    f32x4 xv[XV], gv[XV];
    if (EMBED) {
        const uint32_t id = embed_ids[0];
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            xv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (id < (uint32_t)vocab) {
                const WT* src = table + (int64_t)id * K + (tid + i * 256) * 4;
                if (BF16) {
                    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 r = *reinterpret_cast<const u32x2*>(src);
                    xv[i] = f32x4{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xFFFF0000u), __uint_as_float(r[1] << 16),
                                  __uint_as_float(r[1] & 0xFFFF0000u)};
                } else {
                    xv[i] = *reinterpret_cast<const f32x4*>(src);
                }
            }
        }
        if (blockIdx.x == 0 && x_raw_out) {
#pragma unroll
            for (int i = 0; i < XV; ++i) *reinterpret_cast<f32x4*>(x_raw_out + (tid + i * 256) * 4) = xv[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < XV; ++i) xv[i] = *reinterpret_cast<const f32x4*>(X + (tid + i * 256) * 4);
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) gv[i] = *reinterpret_cast<const f32x4*>(gamma + (tid + i * 256) * 4);
    const int p = pos_ptr ? *pos_ptr : pos;
    const int col = kind == 0 ? n_a : (kind == 1 ? n_a - q_dim : n_a - q_dim - kv_dim);
    const int ri = kind == 2 ? 0 : col % head_dim;  // < half
    const float ba = bias ? bias[n_a] : 0.0f, bb = bias ? bias[n_b] : 0.0f;
    const float cs = cos_t[(int64_t)p * half + ri], sn = sin_t[(int64_t)p * half + ri];
    u32x4 raw[2][CH][LOADS_PER_PIECE];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const char* row = reinterpret_cast<const char*>(W + (int64_t)(r == 0 ? n_a : n_b) * K);
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int l = 0; l < LOADS_PER_PIECE; ++l)
                raw[r][c][l] = load_nt16(row + ((size_t)(c * 64 + lane) * 8) * sizeof(WT) + l * 16);
    }
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < XV; ++i) ss += (xv[i][0] * xv[i][0] + xv[i][1] * xv[i][1]) + (xv[i][2] * xv[i][2] + xv[i][3] * xv[i][3]);
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)K + eps);
#pragma unroll
    for (int i = 0; i < XV; ++i) {
#pragma unroll
        for (int c = 0; c < 4; ++c) xv[i][c] = (xv[i][c] / rms) * gv[i][c];
        *reinterpret_cast<f32x4*>(xs + (tid + i * 256) * 4) = xv[i];
    }
    __syncthreads();
    float acc[2] = {0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const f32x4 xa = *reinterpret_cast<const f32x4*>(xs + (c * 64 + lane) * 8);
        const f32x4 xb = *reinterpret_cast<const f32x4*>(xs + (c * 64 + lane) * 8 + 4);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (BF16) {
                acc[r] = dot8_bf16(raw[r][c][0], xa, xb, acc[r]);
            } else {
                const f32x4 wa = __builtin_bit_cast(f32x4, raw[r][c][0]);
                const f32x4 wb = __builtin_bit_cast(f32x4, raw[r][c][LOADS_PER_PIECE - 1]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[r] = fmaf(xa[e], wa[e], acc[r]);
                    acc[r] = fmaf(xb[e], wb[e], acc[r]);
                }
            }
        }
    }
    const float va = wave_sum(acc[0]) + ba, vb = wave_sum(acc[1]) + bb;
    if (lane != 0 || my >= tasks) return;
    if (kind == 2) {
        Vc[(int64_t)p * kv_dim + col] = va;
        Vc[(int64_t)p * kv_dim + col + 1] = vb;
        return;
    }
    float* out = kind == 0 ? Q : Kc + (int64_t)p * kv_dim;
    out[col] = va * cs - vb * sn;  // rope/mod.rs:156-176
    out[col + half] = va * sn + vb * cs;
}

// In-place rotation of `rows` rows of [n_heads * d] (rope/mod.rs:156-176): pairs (i, i + d/2), position =
// (*pos_ptr | pos) + row; x may start at row (*row_off_ptr | row_off) of a cache.
__global__ __launch_bounds__(256) void rope_kernel(float* __restrict__ x, int64_t ldx, int rows, int n_heads, int head_dim,
                                                   const float* __restrict__ cos_t, const float* __restrict__ sin_t, int pos,
                                                   const int* __restrict__ pos_ptr, int at_cache_row)
{
    const int half = head_dim >> 1;
    const int base = pos_ptr ? *pos_ptr : pos;
    const int total = rows * n_heads * half;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int i = idx % half;
        const int h = (idx / half) % n_heads;
        const int r = idx / (half * n_heads);
        const int p = base + r;
        float* row = x + (int64_t)(at_cache_row ? p : r) * ldx + h * head_dim;
        const float c = cos_t[(int64_t)p * half + i], s = sin_t[(int64_t)p * half + i];
        const float x0 = row[i], x1 = row[i + half];
        row[i] = x0 * c - x1 * s;
        row[i + half] = x0 * s + x1 * c;
    }
}

// out[r, :] = (x[r, :] / sqrt(mean(x^2) + eps)) * gamma   (rms_norm.rs:19-27); one wave per row.
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, float eps,
                                                      int rows, int hidden, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* row = x + (int64_t)r * hidden;
    float s = 0.0f;
    for (int i = lane; i < hidden; i += 64) s = fmaf(row[i], row[i], s);
    const float rms = sqrtf(wave_sum(s) / (float)hidden + eps);
    for (int i = lane; i < hidden; i += 64) out[(int64_t)r * hidden + i] = (row[i] / rms) * gamma[i];
}

// The same with one 256-thread workgroup per row and 16-byte loads (hidden % 4 == 0).
__global__ __launch_bounds__(256) void rmsnorm_block_kernel(const float* __restrict__ x, const float* __restrict__ gamma, float eps,
                                                            int hidden, float* __restrict__ out)
{
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = x + (int64_t)blockIdx.x * hidden;
    const int h4 = hidden >> 2;
    float s = 0.0f;
    for (int i = tid; i < h4; i += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + i * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) s = fmaf(v[c], v[c], s);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)hidden + eps);
    for (int i = tid; i < h4; i += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(row + i * 4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + i * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (v[c] / rms) * g[c];
        *reinterpret_cast<f32x4*>(out + (int64_t)blockIdx.x * hidden + i * 4) = v;
    }
}

template <typename WT>
__global__ __launch_bounds__(256) void llm_embed_kernel(const uint32_t* __restrict__ ids, int hidden, int vocab,
                                                        const WT* __restrict__ table, float* __restrict__ out)
{
    const int s = blockIdx.x;
    const uint32_t id = ids[s];
    for (int i = threadIdx.x; i < hidden / 8; i += 256) {
        F8 v;
#pragma unroll
        for (int c = 0; c < 8; ++c) v.v[c] = 0.0f;
        if (id < (uint32_t)vocab) v = load8(table + (int64_t)id * hidden, i);
#pragma unroll
        for (int c = 0; c < 8; ++c) out[(int64_t)s * hidden + i * 8 + c] = v.v[c];
    }
}

__device__ __forceinline__ unsigned long long argmax_key(float v, int idx)
{
    uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);  // -0.0 == +0.0 (partial_cmp): one key for both, the later index wins
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // larger float -> larger uint
    if (v != v) u = 0;                               // NaN lowest
    return ((unsigned long long)u << 32) | (uint32_t)idx;  // equal values: the LAST index wins (Iterator::max_by)
}

// The largest key of the wave, in every lane (butterfly).
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long key)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, kWave);
        key = o > key ? o : key;
    }
    return key;
}

// The largest key of a workgroup of 256 threads, in thread 0 only: the wave butterfly, then the four waves through red[4] (LDS).
__device__ __forceinline__ unsigned long long block_max_key(unsigned long long key, unsigned long long* red)
{
    key = wave_max_key(key);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) key = red[w] > key ? red[w] : key;
    return key;
}

// Arg-max of row `first_row + blockIdx.y` of logits [., ld] into best[row], the last maximum wins (argmax_key); the x blocks
// stride over the row.  Every pick is a grid over this kernel: launch_argmax (one row), launch_lane_pick (live = the lanes'
// flags: a lane that is not live is not scanned and its slot not touched), launch_lookup_pick (the rows of a verify block).
__global__ __launch_bounds__(256) void argmax_partial_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int first_row,
                                                             const int* __restrict__ live, unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long red[4];
    const int r = first_row + blockIdx.y;
    if (live && !live[r]) return;  // (uniform per workgroup, before the barrier)
    const float* row = logits + (int64_t)r * ld;
    unsigned long long key = 0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) {
        const unsigned long long k = argmax_key(row[i], i);
        key = k > key ? k : key;
    }
    key = block_max_key(key, red);
    if (threadIdx.x == 0) atomicMax(best + r, key);
}

// Publishes the winner, resets the accumulator, and (graph replay) appends the token and advances the counters.
__global__ void argmax_finalize_kernel(unsigned long long* __restrict__ best, int32_t* __restrict__ out,
                                       int32_t* __restrict__ history, int* __restrict__ count, int* __restrict__ pos)
{
    const int tok = (int)(uint32_t)(*best & 0xFFFFFFFFull);
    *best = 0ull;
    *out = tok;
    if (history) {
        history[*count] = tok;
        *count += 1;
        *pos += 1;
    }
}

// Prompt-row projections on the fp32 matrix cores: Y[M, N] = A[M, K] . W[N, K]^T (+ bias) (+ R), W in f32 (bf16 weights
// take the bf16 matrix cores: launch_prefill_tiles_bf16w).  The encoder's 128 x 128 GEMM (gemm.hip) is sized for 10^5 rows; a prompt has 10^2..10^3, where one
// 128 x 128 x 2048 tile keeps a CU busy for ~110 us while most CUs have no tile at all.  So: 64 x 64 block tiles
// (4 waves, one 32 x 32 MFMA tile each) -- 4x more workgroups of a quarter the work --, BK = 32, operands
// double-buffered in LDS with the next tile's global loads in flight during the MFMAs.  v_mfma_f32_32x32x2_f32 is an exact k-ordered f32 fma
// chain, so the arithmetic class is the GEMV's; only the summation order differs.
constexpr int PG_BM = 64, PG_BN = 64, PG_BK = 32, PG_STRIDE = PG_BK + 4;

template <bool RESIDUAL>
__global__ __launch_bounds__(256) void prefill_gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ W,
                                                           const float* __restrict__ bias, const float* R, int64_t ldr, float* Y,
                                                           int64_t ldy, int M, int N, int K, int m_tiles, int ksplit,
                                                           float* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) float sA[2][PG_BM * PG_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[2][PG_BN * PG_STRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs; give every XCD one contiguous run of tiles
    // (row tiles fastest), so the tiles sharing a weight panel sit behind the same L2.
    const int64_t nwg = gridDim.x;
    const int64_t xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int64_t q8 = nwg / 8, r8 = nwg % 8;
    const int64_t bid0 = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    // ksplit > 1 (short prompts: too few tiles for 256 CUs): slice ks of the K range, fastest index, so the slices of a
    // tile run side by side; the partial tiles go to P[ks][M][N] and prefill_splitk_reduce_kernel adds them in order.
    const int ks = (int)(bid0 % ksplit);
    const int64_t bid = bid0 / ksplit;
    const int m0 = (int)(bid % m_tiles) * PG_BM;
    const int n0 = (int)(bid / m_tiles) * PG_BN;
    const int k_len = K / ksplit, k_begin = ks * k_len;

    // A: 64 x 32 floats = 512 float4, two per thread.  W the same.
    const int a_row = tid >> 3, a_c4 = tid & 7;
    const float* a_ptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a_ptr[i] = A + (int64_t)min(m0 + a_row + 32 * i, M - 1) * lda + a_c4 * 4;
    const int b_row = a_row, b_c = a_c4 * 4;
    const float* b_ptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b_ptr[i] = W + (int64_t)min(n0 + b_row + 32 * i, N - 1) * K + b_c;
    f32x4 ga[2], gb[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
#pragma unroll
        for (int i = 0; i < 2; ++i) gb[i] = *reinterpret_cast<const f32x4*>(b_ptr[i] + k0);
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&sA[stage][(a_row + 32 * i) * PG_STRIDE + a_c4 * 4]) = ga[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&sB[stage][(b_row + 32 * i) * PG_STRIDE + b_c]) = gb[i];
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nk = k_len / PG_BK;
    const int fa = (wr * 32 + l31) * PG_STRIDE + half * 4, fb = (wc * 32 + l31) * PG_STRIDE + half * 4;
    load(k_begin);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load(k_begin + (kt + 1) * PG_BK);
#pragma unroll
        for (int kk = 0; kk < PG_BK / 8; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&sA[cur][fa + kk * 8]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&sB[cur][fb + kk * 8]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
        }
        if (kt + 1 < nk) store(cur ^ 1);
        __syncthreads();
    }
    const int col = n0 + wc * 32 + l31;
    if (col < N) {
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

// Y = sum over the K slices (in slice order) + bias + residual: the epilogue of prefill_gemm_kernel for split launches.
__global__ __launch_bounds__(256) void prefill_splitk_reduce_kernel(const float* __restrict__ P, int ksplit, const float* __restrict__ bias,
                                                                    const float* R, int64_t ldr, float* Y, int64_t ldy, int M, int N,
                                                                    float* G)
{
    const int n4 = N >> 2;
    const int64_t total = (int64_t)M * n4, slab = (int64_t)M * N;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / n4;
        const int col = (int)(i - row * n4) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(P + row * N + col);
        for (int s = 1; s < ksplit; ++s) v += *reinterpret_cast<const f32x4*>(P + s * slab + row * N + col);
        if (bias) v += *reinterpret_cast<const f32x4*>(bias + col);
        if (R) v += *reinterpret_cast<const f32x4*>(R + row * ldr + col);
        if (G) {  // this GEMM is the SwiGLU `up`: the gate buffer becomes silu(gate) * up (swiglu.rs:32-57)
            const f32x4 g = *reinterpret_cast<const f32x4*>(G + row * ldy + col);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (g[c] / (1.0f + expf(-g[c]))) * v[c];
            *reinterpret_cast<f32x4*>(G + row * ldy + col) = v;
        } else {
            *reinterpret_cast<f32x4*>(Y + row * ldy + col) = v;
        }
    }
}

// Causal grouped-query attention for a block of prompt rows against the KV cache (decoder_attention.rs:99-160 with the
// causal mask of utils/masks.rs:103-113), flash style: one workgroup per (32 query rows, head), 64-key tiles of K and V
// staged in LDS, running (max, sum, output) per query -- the [rows, keys] score matrix never exists.  8 threads per
// query: each scores 8 keys of the tile (keys kg, kg+8, ...: neighbouring threads read neighbouring K rows) and owns
// head_dim / 8 output columns.  Masked keys contribute exactly 0, as exp(-1e9 - max) does in the reference.
constexpr int PA_Q = 32, PA_K = 64;

template <int DPT>
__global__ __launch_bounds__(256) void prefill_attention_kernel(const float* __restrict__ q, int64_t ldq, int rows,
                                                                const float* __restrict__ K, int64_t ldk,
                                                                const float* __restrict__ V, int64_t ldv, int base, int kv_group,
                                                                float scale, float* __restrict__ ctx, int64_t ldc)
{
    constexpr int D = 8 * DPT, LD = D + 4;
    extern __shared__ __attribute__((aligned(16))) float pa_smem[];
    float* sQ = pa_smem;               // [PA_Q][LD]
    float* sK = sQ + PA_Q * LD;        // [PA_K][LD]
    float* sV = sK + PA_K * LD;        // [PA_K][LD]
    float* sP = sV + PA_K * LD;        // [PA_Q][PA_K + 4]
    const int tid = threadIdx.x, qi = tid >> 3, kg = tid & 7;
    const int h = blockIdx.y, hk = h / kv_group;
    const int q0 = blockIdx.x * PA_Q;
    const int q_row = q0 + qi;
    const bool valid = q_row < rows;
    const int limit = base + q_row;                                   // last visible key of this query
    const int last_key = base + min(rows, q0 + PA_Q) - 1;             // last key any query of the block sees
    for (int i = tid; i < PA_Q * (D / 4); i += 256) {
        const int r = i / (D / 4), c4 = i - r * (D / 4);
        const int row = min(q0 + r, rows - 1);
        *reinterpret_cast<f32x4*>(sQ + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(q + (int64_t)row * ldq + h * D + c4 * 4);
    }
    float m_run = -INFINITY, l_run = 0.0f;
    float o[DPT];
#pragma unroll
    for (int c = 0; c < DPT; ++c) o[c] = 0.0f;
    for (int k0 = 0; k0 <= last_key; k0 += PA_K) {
        __syncthreads();  // previous tile fully consumed (and sQ written, first trip)
        for (int i = tid; i < PA_K * (D / 4); i += 256) {
            const int r = i / (D / 4), c4 = i - r * (D / 4);
            const int key = min(k0 + r, last_key);
            *reinterpret_cast<f32x4*>(sK + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(K + (int64_t)key * ldk + hk * D + c4 * 4);
            *reinterpret_cast<f32x4*>(sV + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(V + (int64_t)key * ldv + hk * D + c4 * 4);
        }
        __syncthreads();
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int c4 = 0; c4 < D / 4; ++c4) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(sQ + qi * LD + c4 * 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 kv = *reinterpret_cast<const f32x4*>(sK + (kg + 8 * j) * LD + c4 * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[j] = fmaf(qv[c], kv[c], acc[j]);
            }
        }
        float tile_max = -INFINITY;
        bool vis[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            acc[j] *= scale;
            vis[j] = valid && (k0 + kg + 8 * j) <= limit;
            if (vis[j]) tile_max = fmaxf(tile_max, acc[j]);
        }
        tile_max = group8_max_asc(tile_max);  // (the query's 8 lanes)
        const float m_new = fmaxf(m_run, tile_max);
        float psum = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = vis[j] ? expf(acc[j] - m_new) : 0.0f;
            psum += p;
            sP[qi * (PA_K + 4) + kg + 8 * j] = p;
        }
        psum = group8_sum_asc(psum);
        const float alpha = (m_new == -INFINITY || m_run == -INFINITY) ? (m_run == -INFINITY ? 0.0f : 1.0f) : expf(m_run - m_new);
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int c = 0; c < DPT; ++c) o[c] *= alpha;
        m_run = m_new;
        __syncthreads();  // the tile's probabilities are in LDS
        for (int j = 0; j < PA_K; ++j) {
            const float p = sP[qi * (PA_K + 4) + j];
#pragma unroll
            for (int c = 0; c < DPT; ++c) o[c] = fmaf(p, sV[j * LD + kg * DPT + c], o[c]);
        }
    }
    if (valid) {
        const float inv = l_run > 0.0f ? 1.0f / l_run : 0.0f;
#pragma unroll
        for (int c = 0; c < DPT; ++c) ctx[(int64_t)q_row * ldc + h * D + kg * DPT + c] = o[c] * inv;
    }
}

// Prefill: silu(gate) * up over [rows, inter] (swiglu.rs:32-57).
__global__ __launch_bounds__(256) void swiglu_mul_kernel(float* __restrict__ gate, const float* __restrict__ up, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 g = *reinterpret_cast<const f32x4*>(gate + i * 4);
        const f32x4 u = *reinterpret_cast<const f32x4*>(up + i * 4);
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = (g[c] / (1.0f + expf(-g[c]))) * u[c];
        *reinterpret_cast<f32x4*>(gate + i * 4) = g;
    }
}

}  // namespace

LlmGemvRoute llm_gemv_route(const LlmGemvArgs& a)
{
    LlmGemvRoute r;
    const bool norm = a.gamma != nullptr;
    // Staging the row in LDS pays when it also has to be normalised (otherwise every wave redoes the statistics); plain
    // projections keep the one-wave-per-column kernel, whose 4x larger grid hides latency better.
    // One row, K = 2048 / 4096 / 8192: the weight-streaming kernel.
    if (!a.layernorm && a.rows == 1 && a.seg_q == 0 && llm_gemv_streams(a.k, a.W, a.W2)) {
        const int ch = a.k / 512;
        const int nm = a.swiglu ? 2 : 1, lpp = a.bf16 ? 1 : 2;
        // 16 loads per lane in flight where that still leaves >= 8 waves per CU, else one row per wave
        const bool wide = a.n_out / stream_rows_per_batch(ch, lpp, nm, true) >= 2048;
        const int rb = stream_rows_per_batch(ch, lpp, nm, wide);
        const int batches = (a.n_out + rb - 1) / rb;
        // 8-wave workgroups where they still cover every CU and staging the input row is the larger cost (a long row, or the
        // attention slabs to merge: each workgroup stages the whole row, so fewer, larger ones re-read it less; measured on
        // the 1B shape: down-proj 8.0 -> 7.6 us, output projection with the merge 6.4 -> 4.9 us, gate/up 12.8 -> 13.2 us);
        // the layer's projections get one batch per wave, the vocabulary head loops
        const bool big = batches >= 2048 && (ch >= 16 || a.att_splits > 0);
        const int wpw = big ? 8 : 4;
        const bool loop = (batches + wpw - 1) / wpw > 4096 / wpw;
        r.kernel = LLM_GEMV_STREAM;
        r.ch = ch;
        r.wide = (wide || loop) ? 1 : 0;  // the looping form is instantiated with the 16-load batches only
        r.threads = big ? 512 : 256;
        r.loop = loop ? 1 : 0;
        r.rows_per_batch = stream_rows_per_batch(ch, lpp, nm, r.wide != 0);
        r.workgroups = loop ? 2048 / wpw : std::max(1, (batches + wpw - 1) / wpw);
        return r;
    }
    // LayerNorm (GPT-2) takes three kernels, each instantiated for the one combination it serves: one row, k <= 2048, the
    // c_fc stage (LayerNorm + GELU) -> split-K; one row, the Q|K|V stage (LayerNorm, cache segments) -> the LDS-staged
    // kernel; everything else -> the multi-row kernel.
    const bool ln_splitk = a.layernorm && a.rows == 1 && a.gelu_tanh && a.seg_q == 0 && a.k <= 2048;
    const bool ln_one = a.layernorm && a.rows == 1 && !a.gelu_tanh && a.k <= G1_MAX_K;
    const bool rms_splitk = !a.layernorm && a.rows == 1 && a.seg_q == 0 && a.k <= SK_MAX_CHUNKS * 2048;
    const bool rms_one = !a.layernorm && a.rows == 1 && norm && a.k <= G1_MAX_K;
    if (ln_splitk || (!ln_one && rms_splitk)) {
        const bool wide = !ln_splitk && a.k >= 8192;  // 16 waves per workgroup
        const int threads = wide ? 1024 : 256;
        const int chunks = (a.k / 8 + threads - 1) / threads;
        const int ch = chunks <= 1 ? 1 : (chunks <= 2 ? 2 : (chunks <= 4 ? 4 : 8));
        r.kernel = LLM_GEMV_SPLITK;
        r.ch = ln_splitk ? 1 : (wide && ch > 2 ? 2 : ch);
        r.wide = wide ? 1 : 0;
        r.threads = threads;
        r.rows_per_batch = SK_OPW;
        r.workgroups = (a.n_out + SK_OPW - 1) / SK_OPW;
        return r;
    }
    if (ln_one || rms_one) {
        r.kernel = LLM_GEMV_ONE;
        r.rows_per_batch = G1_OPW;
        r.workgroups = (a.n_out + 4 * G1_OPW - 1) / (4 * G1_OPW);
        return r;
    }
    r.kernel = LLM_GEMV_GENERIC;
    r.workgroups = (a.n_out + 3) / 4;
    return r;
}

template <typename WT>
static hipError_t launch_gemv_t(const LlmGemvArgs& a, hipStream_t stream)
{
    const WT* W = static_cast<const WT*>(a.W);
    const WT* W2 = static_cast<const WT*>(a.W2);
    const bool norm = a.gamma != nullptr;
    const LlmGemvRoute rt = llm_gemv_route(a);  // which kernel, in which form: every decision below is read from it
    // The (epilogue, norm) pairs the callers request (launch_llm_gemv rejects every other one), and the only ones
    // instantiated; each route below takes those of them it can reach:
    //   (LE_NONE, NK_RMS)        RMSNorm + Q|K|V (llm.cpp pass: prompt rows, or one row wider than 8192), the decode step's head
    //   (LE_NONE, NK_NONE)       the vocabulary head after the final norm (pass, pass_gpt2, prefill_rows)
    //   (LE_RESIDUAL, NK_NONE)   o / down projection + residual (pass, pass_gpt2)
    //   (LE_SWIGLU, NK_RMS)      RMSNorm + gate / up + SwiGLU (pass)
    //   (LE_NONE, NK_LN)         LayerNorm + Q|K|V (pass_gpt2)
    //   (LE_GELU_TANH, NK_LN)    LayerNorm + c_fc + GELU-tanh (pass_gpt2)
#define KJ_RMS_PAIRS(LAUNCH)                                                                                                         \
    do {                                                                                                                             \
        if (a.swiglu) LAUNCH(LE_SWIGLU, NK_RMS);                                                                                     \
        else if (a.R) LAUNCH(LE_RESIDUAL, NK_NONE);                                                                                  \
        else if (norm) LAUNCH(LE_NONE, NK_RMS);                                                                                      \
        else LAUNCH(LE_NONE, NK_NONE);                                                                                               \
    } while (0)
    // Staging the row in LDS pays when it also has to be normalised (otherwise every wave redoes the statistics); plain
    // projections keep the one-wave-per-column kernel, whose 4x larger grid hides latency better.
    // One row, K = 2048 / 4096 / 8192: the weight-streaming kernel.
    if (rt.kernel == LLM_GEMV_STREAM) {
        // (the rule -- 16 loads per lane in flight, 8-wave workgroups, the looping head -- is llm_gemv_route's)
        const int ch = rt.ch, wgs = rt.workgroups;
        const bool wide = rt.wide != 0, loop = rt.loop != 0, big = rt.threads == 512;
#define KJ_ST4(EPI, NORM, CH, WIDE, LOOP, THREADS)                                                                                   \
    hipLaunchKernelGGL((llm_gemv_stream_kernel<WT, EPI, NORM != NK_NONE, CH, WIDE, LOOP, THREADS>), dim3((unsigned)wgs), dim3(THREADS), \
                       0, stream, a.X, a.gamma, a.eps, W, W2, a.bias, a.R, a.n_out, a.Y0, 0, 0, a.norm_out)
#define KJ_ST3(EPI, NORM, CH, WIDE, LOOP)                                                                                            \
    do {                                                                                                                             \
        if (big) KJ_ST4(EPI, NORM, CH, WIDE, LOOP, 512);                                                                             \
        else KJ_ST4(EPI, NORM, CH, WIDE, LOOP, 256);                                                                                 \
    } while (0)
#define KJ_ST_ATT2(CH, WIDE, THREADS, ATT)                                                                                           \
    hipLaunchKernelGGL((llm_gemv_stream_kernel<WT, LE_RESIDUAL, false, CH, WIDE, false, THREADS, ATT>), dim3((unsigned)wgs),         \
                       dim3(THREADS), 0, stream, a.X, a.gamma, a.eps, W, W2, a.bias, a.R, a.n_out, a.Y0, a.att_splits, a.att_head_dim, \
                       nullptr)
#define KJ_ST_ATT(CH, ATT)                                                                                                           \
    do {                                                                                                                             \
        if (big && wide) KJ_ST_ATT2(CH, true, 512, ATT);                                                                             \
        else if (big) KJ_ST_ATT2(CH, false, 512, ATT);                                                                               \
        else if (wide) KJ_ST_ATT2(CH, true, 256, ATT);                                                                               \
        else KJ_ST_ATT2(CH, false, 256, ATT);                                                                                        \
    } while (0)
        if (a.att_splits > 0) {  // the context row arrives as attention slabs
            if (!llm_gemv_merges_attention(a.k, a.att_splits, a.att_head_dim) || !a.R || norm || a.swiglu || loop) return hipErrorInvalidValue;
            if (ch == 4) KJ_ST_ATT(4, 8);
            else KJ_ST_ATT(8, 4);
            return hipGetLastError();
        }
#define KJ_ST2(EPI, NORM, CH)                                                                                                        \
    do {                                                                                                                             \
        if (loop) KJ_ST3(EPI, NORM, CH, true, true);                                                                                 \
        else if (wide) KJ_ST3(EPI, NORM, CH, true, false);                                                                           \
        else KJ_ST3(EPI, NORM, CH, false, false);                                                                                    \
    } while (0)
#define KJ_ST1(EPI, NORM)                                                                                                            \
    do {                                                                                                                             \
        if (ch == 4) KJ_ST2(EPI, NORM, 4);                                                                                           \
        else if (ch == 8) KJ_ST2(EPI, NORM, 8);                                                                                      \
        else KJ_ST2(EPI, NORM, 16);                                                                                                  \
    } while (0)
        KJ_RMS_PAIRS(KJ_ST1);
#undef KJ_ST1
#undef KJ_ST2
#undef KJ_ST3
#undef KJ_ST4
#undef KJ_ST_ATT
#undef KJ_ST_ATT2
        return hipGetLastError();
    }
    // LayerNorm (GPT-2) takes three kernels, each instantiated for the one combination it serves: one row, k <= 2048, the
    // c_fc stage (LayerNorm + GELU) -> split-K; one row, the Q|K|V stage (LayerNorm, cache segments) -> the LDS-staged
    // kernel; everything else -> the multi-row kernel below.
    if (rt.kernel == LLM_GEMV_SPLITK && a.layernorm) {
        hipLaunchKernelGGL((llm_gemv_splitk_kernel<WT, LE_GELU_TANH, NK_LN, 1, 4>), dim3((unsigned)rt.workgroups), dim3(256),
                           0, stream, a.X, a.gamma, a.eps, W, W2, a.bias, a.R, a.n_out, a.k, a.Y0, a.beta);
        return hipGetLastError();
    }
    const dim3 grid1((unsigned)((a.n_out + 4 * G1_OPW - 1) / (4 * G1_OPW)));  // (= rt.workgroups where the route is this kernel)
    const size_t lds1 = (size_t)a.k * sizeof(float);
#define KJ_LLM1(EPI, NORM)                                                                                                            \
    do {                                                                                                                              \
        auto kern = llm_gemv1_kernel<WT, EPI, NORM>;                                                                                  \
        if (lds1 > 48 * 1024) {                                                                                                       \
            const hipError_t e = allow_dynamic_lds(kern, lds1);                                                                       \
            if (e != hipSuccess) return e;                                                                                            \
        }                                                                                                                             \
        hipLaunchKernelGGL(kern, grid1, dim3(256), lds1, stream, a.X, a.gamma, a.eps, W, W2, a.bias, a.R, a.n_out, a.k, a.seg_q,      \
                           a.seg_kv, a.Y0, a.Y1, a.Y2, a.ldy12, a.row_off, a.row_off_ptr, a.beta);                                    \
    } while (0)
    if (rt.kernel == LLM_GEMV_ONE && a.layernorm) {
        KJ_LLM1(LE_NONE, NK_LN);
        return hipGetLastError();
    }
    if (rt.kernel == LLM_GEMV_SPLITK) {
        // Long rows (down-proj: k = 8192 .. 14336) are spread over 16 waves per workgroup: a quarter of the loads per lane,
        // four times the waves in flight, at the same two columns per workgroup.
        const bool wide = rt.wide != 0;
        const int chunks = rt.ch;
        const dim3 gridk((unsigned)rt.workgroups);
#define KJ_SK3(EPI, NORM, CH, NW)                                                                                                     \
    hipLaunchKernelGGL((llm_gemv_splitk_kernel<WT, EPI, NORM, CH, NW>), gridk, dim3(64 * NW), 0, stream, a.X, a.gamma, a.eps, W, W2,  \
                       a.bias, a.R, a.n_out, a.k, a.Y0, a.beta)
#define KJ_SK2(EPI, NORM, CH)                                                                                                         \
    do {                                                                                                                              \
        if (wide) KJ_SK3(EPI, NORM, (CH > 2 ? 2 : CH), 16);                                                                           \
        else KJ_SK3(EPI, NORM, CH, 4);                                                                                                \
    } while (0)
#define KJ_SK1(EPI, NORM)                                                                                                             \
    do {                                                                                                                              \
        if (chunks <= 1) KJ_SK2(EPI, NORM, 1);                                                                                        \
        else if (chunks <= 2) KJ_SK2(EPI, NORM, 2);                                                                                   \
        else if (chunks <= 4) KJ_SK2(EPI, NORM, 4);                                                                                   \
        else KJ_SK2(EPI, NORM, 8);                                                                                                    \
    } while (0)
        KJ_RMS_PAIRS(KJ_SK1);
#undef KJ_SK1
#undef KJ_SK2
#undef KJ_SK3
        return hipGetLastError();
    }
    if (rt.kernel == LLM_GEMV_ONE) {
        if (a.swiglu) KJ_LLM1(LE_SWIGLU, NK_RMS);
        else KJ_LLM1(LE_NONE, NK_RMS);
        return hipGetLastError();
    }
#undef KJ_LLM1
    const dim3 grid((unsigned)rt.workgroups);
#define KJ_LLM(EPI, NORM)                                                                                                       \
    hipLaunchKernelGGL((llm_gemv_kernel<WT, EPI, NORM>), grid, dim3(256), 0, stream, a.X, a.ldx, a.rows, a.gamma, a.eps, W, W2,  \
                       a.bias, a.R, a.ldr, a.n_out, a.k, a.seg_q, a.seg_kv, a.Y0, a.ldy0, a.Y1, a.Y2, a.ldy12, a.row_off,       \
                       a.row_off_ptr, a.beta)
    if (a.layernorm) {  // the GPT-2 stages that reach here: 2-8 rows, or a projection too wide for the kernels above
        if (a.gelu_tanh) KJ_LLM(LE_GELU_TANH, NK_LN);
        else KJ_LLM(LE_NONE, NK_LN);
    } else {
        KJ_RMS_PAIRS(KJ_LLM);
    }
#undef KJ_LLM
#undef KJ_RMS_PAIRS
    return hipGetLastError();
}

int prefill_gemm_ksplit(int M, int N, int K)
{
    const int tiles = ((M + PG_BM - 1) / PG_BM) * ((N + PG_BN - 1) / PG_BN);
    int s = 1;
    // up to 8 slices of >= 128 columns of K while the launch stays within ~4 workgroups per CU
    while (s < 8 && tiles * s * 2 <= 1024 && K % (s * 2 * PG_BK) == 0 && K / (s * 2) >= 128) s *= 2;
    return s;
}

size_t prefill_gemm_scratch_floats(int max_rows, int max_n)
{
    // ksplit * tiles <= 1024 tiles of 64 x 64, or one unsplit slab when there are more tiles than that
    (void)max_rows;
    (void)max_n;
    return (size_t)1024 * PG_BM * PG_BN;
}

int prefill_gemm_launch_ksplit(const float* bias, const float* R, int64_t ldr, const float* Y, int64_t ldy, int M, int N, int K,
                               const float* split_scratch)
{
    // the reduce kernel moves float4s: a scratch, N and every row stride multiples of 4, every base 16-byte aligned
    if (split_scratch && (N & 3) == 0 && (ldy & 3) == 0 && (!R || (ldr & 3) == 0) && (reinterpret_cast<uintptr_t>(Y) & 15) == 0 &&
        (!R || (reinterpret_cast<uintptr_t>(R) & 15) == 0) && (!bias || (reinterpret_cast<uintptr_t>(bias) & 15) == 0))
        return prefill_gemm_ksplit(M, N, K);
    return 1;
}

hipError_t launch_prefill_splitk_reduce(const float* partials, int ksplit, const float* bias, const float* R, int64_t ldr, float* Y, int64_t ldy,
                                        int M, int N, float* silu_gate, hipStream_t stream)
{
    const int64_t total = (int64_t)M * (N / 4);
    const unsigned blocks = (unsigned)std::min<int64_t>(2048, (total + 255) / 256);
    hipLaunchKernelGGL(prefill_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, stream, partials, ksplit, bias, R, ldr, Y, ldy, M, N, silu_gate);
    return hipGetLastError();
}

hipError_t launch_prefill_gemm(const float* A, int64_t lda, const void* W, int bf16, const float* bias, const float* R, int64_t ldr, float* Y,
                               int64_t ldy, int M, int N, int K, hipStream_t stream, float* split_scratch, float* silu_gate)
{
    if (M <= 0 || N <= 0) return hipSuccess;
    if (K % PG_BK || lda % 4 || (reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(W) & 15)) return hipErrorInvalidValue;
    if (silu_gate && (ldy != N || (N & 3) || (reinterpret_cast<uintptr_t>(silu_gate) & 15))) return hipErrorInvalidValue;
    const int m_tiles = (M + PG_BM - 1) / PG_BM, n_tiles = (N + PG_BN - 1) / PG_BN;
    const int ksplit = prefill_gemm_launch_ksplit(bias, R, ldr, Y, ldy, M, N, K, split_scratch);
    const dim3 grid((unsigned)(m_tiles * n_tiles * ksplit));
#define KJ_PG(RES)                                                                                                                  \
    hipLaunchKernelGGL((prefill_gemm_kernel<RES>), grid, dim3(256), 0, stream, A, lda, static_cast<const float*>(W), bias, R, ldr, Y, ldy, \
                       M, N, K, m_tiles, ksplit, split_scratch)
    if (bf16) {
        // bf16 weights: on the bf16 matrix cores, the activations as three exact bf16 pieces (gemm_split.hip)
        const hipError_t e = launch_prefill_tiles_bf16w((unsigned)(m_tiles * n_tiles * ksplit), A, lda, W, bias, R, ldr, Y, ldy, M, N, K, m_tiles,
                                                        ksplit, split_scratch, stream);
        if (e != hipSuccess) return e;
    } else if (R) {
        KJ_PG(true);
    } else {
        KJ_PG(false);
    }
#undef KJ_PG
    if (ksplit > 1) {
        return launch_prefill_splitk_reduce(split_scratch, ksplit, bias, R, ldr, Y, ldy, M, N, silu_gate, stream);
    } else if (silu_gate) {
        return launch_swiglu_mul(silu_gate, Y, (size_t)M * N, stream);
    }
    return hipGetLastError();
}

namespace {
// bf16 -> f32, eight values per thread (a long prompt's projections run the encoder's f32 tile GEMM on a widened copy)
__global__ __launch_bounds__(256) void widen_bf16_kernel(const uint16_t* __restrict__ src, float* __restrict__ dst, size_t n8)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
        const F8 w = load8(src, (int64_t)i);
        *reinterpret_cast<f32x4*>(dst + i * 8) = f32x4{w.v[0], w.v[1], w.v[2], w.v[3]};
        *reinterpret_cast<f32x4*>(dst + i * 8 + 4) = f32x4{w.v[4], w.v[5], w.v[6], w.v[7]};
    }
}
}  // namespace

hipError_t launch_widen_bf16(const void* src, float* dst, size_t n, hipStream_t stream)
{
    if (n & 7) return hipErrorInvalidValue;
    const size_t n8 = n >> 3;
    hipLaunchKernelGGL(widen_bf16_kernel, dim3((unsigned)std::min<size_t>(4096, (n8 + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint16_t*>(src), dst, n8);
    return hipGetLastError();
}

namespace {
// Causal grouped-query attention of a long prompt block on the fp32 matrix cores (the flash-style kernel above is a vector-ALU
// kernel: 27 TFLOP/s, a quarter of a 2 048-token prompt's time).  Structure of the encoder's attention_kernel (attention.hip):
// a workgroup owns 128 queries of one head (4 waves x 32), walks the keys in chunks of 128 staged in LDS (K row-major, V
// transposed), S^T = K Q^T and O += P V as 32 x 32 x 2 MFMA tiles, online softmax in the exp2 domain with the running
// (max, sum) on lane == query.  Causality: query row i of the block sees keys <= base + i (decoder_attention.rs:99-160,
// utils/masks.rs:103-113 overwrite masked scores with -1e9, whose exp is exactly 0 next to the unmasked diagonal score --
// here they are simply left out); chunks past a workgroup's last query are never visited, a wave skips the chunks past its
// own last query, and only the chunks that straddle a wave's diagonal pay for the per-element test.
constexpr int PM_Q = 128, PM_K = 128;
template <int D>
struct PmSmem {
    static constexpr int K_STRIDE = D + 4, VT_STRIDE = PM_K + 4;
    static constexpr int K_FLOATS = PM_K * K_STRIDE, VT_FLOATS = D * VT_STRIDE;
    static constexpr int BYTES = (K_FLOATS + VT_FLOATS) * 4;
};

template <int D>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void prefill_attention_mfma_kernel(const float* __restrict__ q, int64_t ldq, int rows,
                                                                                       const float* __restrict__ K, int64_t ldk,
                                                                                       const float* __restrict__ V, int64_t ldv, int base,
                                                                                       int kv_group, float scale, float* __restrict__ ctx,
                                                                                       int64_t ldc)
{
    using SM = PmSmem<D>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sK = smem;                  // [128][D + 4]
    float* sVt = smem + SM::K_FLOATS;  // [D][128 + 4]
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    // A query block's work grows with its index (block i walks i + 1 key chunks when nothing is cached).  All workgroups of a
    // launch are resident at once, two per CU, and workgroups L and L + 256 tend to share one: the upper half of the heads
    // walks the blocks in reverse, so the pairs add up to the same work.
    const int h = blockIdx.y, kvh = h / kv_group;
    const int qb = (2 * (int)blockIdx.y >= (int)gridDim.y) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const float* q_base = q + h * D;
    const float* k_base = K + kvh * D;
    const float* v_base = V + kvh * D;

    const int q_wave0 = qb * PM_Q + wid * 32;  // first query row of this wave
    const int q_row = q_wave0 + l31;
    f32x4 qf[D / 8];  // B operand of S^T = K Q^T: lane supplies Q[q][8 kk + 4 half + c]
#pragma unroll
    for (int kk = 0; kk < D / 8; ++kk)
        qf[kk] = q_row < rows ? *reinterpret_cast<const f32x4*>(q_base + (int64_t)q_row * ldq + kk * 8 + half * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x16 o[D / 32];
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.0f;
    float run_max = -INFINITY, run_sum = 0.0f;
    const int n_keys = base + rows;
    const int last_q_wg = min(rows, qb * PM_Q + PM_Q) - 1;     // last query row of the workgroup
    const int last_q_wave = min(rows - 1, q_wave0 + 31);        // (below q_wave0 when the wave has no query: it only helps staging)
    const int n_chunks = (base + last_q_wg) / PM_K + 1;
    const float c1 = scale * 1.4426950408889634f;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const int key0 = ch * PM_K;
        if (ch > 0) __syncthreads();  // everyone done reading the previous chunk
        constexpr int V4_PER_ROW = D / 4;
        for (int f = tid; f < PM_K * V4_PER_ROW; f += 256) {
            const int r = f / V4_PER_ROW, c4 = f % V4_PER_ROW;
            const int key = key0 + r;
            f32x4 kv = f32x4{0.f, 0.f, 0.f, 0.f}, vv = kv;
            if (key < n_keys) {
                kv = *reinterpret_cast<const f32x4*>(k_base + (int64_t)key * ldk + c4 * 4);
                vv = *reinterpret_cast<const f32x4*>(v_base + (int64_t)key * ldv + c4 * 4);
            }
            *reinterpret_cast<f32x4*>(sK + r * SM::K_STRIDE + c4 * 4) = kv;
#pragma unroll
            for (int c = 0; c < 4; ++c) sVt[(c4 * 4 + c) * SM::VT_STRIDE + r] = vv[c];
        }
        __syncthreads();
        if (q_wave0 >= rows || key0 > base + last_q_wave) continue;  // no query here, or every key of the chunk is in this wave's future
        const bool plain = key0 + PM_K - 1 <= base + q_wave0;      // every key visible to every query of the wave

        f32x16 s[4];  // S^T tiles: 4 key tiles x 32 queries, K = D
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kt][r] = 0.0f;
            const float* pk = sK + (kt * 32 + l31) * SM::K_STRIDE + half * 4;
#pragma unroll
            for (int kk = 0; kk < D / 8; ++kk) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(pk + kk * 8);
#pragma unroll
                for (int c = 0; c < 4; ++c) s[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[c], qf[kk][c], s[kt], 0, 0, 0);
            }
        }
        float cmax = -INFINITY;
        if (plain) {
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    s[kt][r] *= c1;
                    cmax = fmaxf(cmax, s[kt][r]);
                }
        } else {
            const int limit = base + q_row;  // this lane's query sees keys <= limit
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = key0 + kt * 32 + acc_row(r, half);
                    const float v = key <= limit ? s[kt][r] * c1 : -INFINITY;
                    s[kt][r] = v;
                    cmax = fmaxf(cmax, v);
                }
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, kWave));
        const float new_max = fmaxf(run_max, cmax);
        // (a lane without a query, or whose keys of this chunk are all in its future, keeps new_max == run_max)
        const float alpha = (run_max == -INFINITY) ? 0.0f : __builtin_amdgcn_exp2f(run_max - new_max);
        float csum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float e = __builtin_amdgcn_exp2f(s[kt][r] - new_max);
                if (new_max == -INFINITY) e = 0.0f;
                s[kt][r] = e;
                csum += e;
            }
        csum += __shfl_xor(csum, 32, kWave);
        run_sum = run_sum * alpha + csum;
        run_max = new_max;
#pragma unroll
        for (int r = 0; r < 16; ++r) {  // O's rows are queries indexed by (reg, half); alpha lives on lane == query
            const float a = __shfl(alpha, acc_row(r, half), kWave);
#pragma unroll
            for (int dt = 0; dt < D / 32; ++dt) o[dt][r] *= a;
        }
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {  // O += P V: A = P (query l31, keys 8 g + 4 half + c), B = V^T[d][key]
            const float* pv = sVt + (dt * 32 + l31) * SM::VT_STRIDE + half * 4;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 vf = *reinterpret_cast<const f32x4*>(pv + kt * 32 + g * 8);
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(s[kt][g * 4 + c], vf[c], o[dt], 0, 0, 0);
                }
        }
    }
    const float inv = run_sum > 0.0f ? 1.0f / run_sum : 1.0f;
    float* out_base = ctx + h * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qq = q_wave0 + acc_row(r, half);
        const float is = __shfl(inv, acc_row(r, half), kWave);
        if (qq < rows) {
#pragma unroll
            for (int dt = 0; dt < D / 32; ++dt) out_base[(int64_t)qq * ldc + dt * 32 + l31] = o[dt][r] * is;
        }
    }
}
}  // namespace

bool prefill_attention_supported(int head_dim) { return head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128; }

int prefill_attention_route(const float* q, int64_t ldq, int rows, const float* K, int64_t ldk, const float* V, int64_t ldv, int head_dim)
{
    // long blocks of 64- / 128-wide heads: the matrix-core kernel
    return rows >= 256 && (head_dim == 64 || head_dim == 128) && (ldq & 3) == 0 && (ldk & 3) == 0 && (ldv & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(V)) & 15) == 0
               ? 1
               : 0;
}

hipError_t launch_prefill_attention(const float* q, int64_t ldq, int rows, const float* K, int64_t ldk, const float* V, int64_t ldv, int base,
                                    int heads, int head_dim, int kv_group, float* ctx, int64_t ldc, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!prefill_attention_supported(head_dim)) return hipErrorInvalidValue;
    if (prefill_attention_route(q, ldq, rows, K, ldk, V, ldv, head_dim) == 1) {
        const dim3 mgrid((unsigned)((rows + PM_Q - 1) / PM_Q), (unsigned)heads);
        const float mscale = 1.0f / sqrtf((float)head_dim);
        const int g = kv_group < 1 ? 1 : kv_group;
        if (head_dim == 64) {
            auto kern = prefill_attention_mfma_kernel<64>;
            const hipError_t e = allow_dynamic_lds(kern, PmSmem<64>::BYTES);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, mgrid, dim3(256), PmSmem<64>::BYTES, stream, q, ldq, rows, K, ldk, V, ldv, base, g, mscale, ctx, ldc);
        } else {
            auto kern = prefill_attention_mfma_kernel<128>;
            const hipError_t e = allow_dynamic_lds(kern, PmSmem<128>::BYTES);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, mgrid, dim3(256), PmSmem<128>::BYTES, stream, q, ldq, rows, K, ldk, V, ldv, base, g, mscale, ctx, ldc);
        }
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((rows + PA_Q - 1) / PA_Q), (unsigned)heads);
    const int LD = head_dim + 4;
    const size_t lds = ((size_t)(PA_Q + 2 * PA_K) * LD + (size_t)PA_Q * (PA_K + 4)) * sizeof(float);
    const float scale = 1.0f / sqrtf((float)head_dim);
#define KJ_PA(DPT)                                                                                                                      \
    do {                                                                                                                                \
        auto kern = prefill_attention_kernel<DPT>;                                                                                      \
        if (lds > 48 * 1024) {                                                                                                          \
            const hipError_t e = allow_dynamic_lds(kern, lds);                                                                          \
            if (e != hipSuccess) return e;                                                                                              \
        }                                                                                                                               \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, q, ldq, rows, K, ldk, V, ldv, base, kv_group < 1 ? 1 : kv_group, scale,  \
                           ctx, ldc);                                                                                                   \
    } while (0)
    switch (head_dim) {
    case 16: KJ_PA(2); break;
    case 32: KJ_PA(4); break;
    case 64: KJ_PA(8); break;
    default: KJ_PA(16); break;
    }
#undef KJ_PA
    return hipGetLastError();
}

hipError_t launch_swiglu_mul(float* gate, const float* up, size_t n, hipStream_t stream)
{
    if (n % 4) return hipErrorInvalidValue;
    const size_t n4 = n / 4;
    const unsigned grid = (unsigned)std::min<size_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(swiglu_mul_kernel, dim3(grid), dim3(256), 0, stream, gate, up, n4);
    return hipGetLastError();
}

bool llm_qkv_rope_embeds(int k, const float* gamma, const void* W, const void* table)
{
    return (k == 2048 || k == 4096 || k == 8192) && gamma && (reinterpret_cast<uintptr_t>(W) & 15) == 0 &&
           (reinterpret_cast<uintptr_t>(table) & 15) == 0;
}

LlmQkvRopeRoute llm_qkv_rope_route(int k, const float* gamma, const void* W, int n_heads, int n_kv_heads, int head_dim,
                                   const uint32_t* embed_ids)
{
    LlmQkvRopeRoute r;
    const int tasks = (n_heads * head_dim + 2 * n_kv_heads * head_dim) / 2;  // pairs of output columns
    if ((k == 2048 || k == 4096 || k == 8192) && gamma && (reinterpret_cast<uintptr_t>(W) & 15) == 0) {
        r.kernel = embed_ids ? LLM_QKV_STREAM_EMBED : LLM_QKV_STREAM;
        r.ch = k / 512;
        r.workgroups = (tasks + 3) / 4;  // one wave per pair
        return r;
    }
    const int chunks = (k / 8 + 255) / 256;
    r.kernel = LLM_QKV_PAIR;
    r.ch = chunks <= 1 ? 1 : (chunks <= 2 ? 2 : 4);
    r.workgroups = tasks;  // one workgroup per pair
    return r;
}

hipError_t launch_llm_qkv_rope(const float* X, const float* gamma, float eps, const void* W, int bf16, const float* bias, int k,
                               int n_heads, int n_kv_heads, int head_dim, const float* cos_t, const float* sin_t, float* Q, float* Kc,
                               float* Vc, int pos, const int* pos_ptr, hipStream_t stream, const uint32_t* embed_ids, const void* table,
                               int vocab, float* x_raw_out)
{
    // (both kernels read gamma: the step is RMSNorm + projection + RoPE, there is no form without the norm)
    if ((k & 7) || k > 8192 || (head_dim & 1) || !gamma) return hipErrorInvalidValue;
    if (embed_ids && !llm_qkv_rope_embeds(k, gamma, W, table)) return hipErrorInvalidValue;
    const LlmQkvRopeRoute rt = llm_qkv_rope_route(k, gamma, W, n_heads, n_kv_heads, head_dim, embed_ids);
    if (rt.kernel != LLM_QKV_PAIR) {
        const dim3 sgrid((unsigned)rt.workgroups);
#define KJ_QKVS(WT, CH)                                                                                                              \
    do {                                                                                                                             \
        if (embed_ids)                                                                                                               \
            hipLaunchKernelGGL((llm_qkv_rope_stream_kernel<WT, CH, true>), sgrid, dim3(256), 0, stream, X, gamma, eps,                \
                               static_cast<const WT*>(W), bias, n_heads, n_kv_heads, head_dim, cos_t, sin_t, Q, Kc, Vc, pos, pos_ptr, \
                               embed_ids, static_cast<const WT*>(table), vocab, x_raw_out);                                          \
        else                                                                                                                         \
            hipLaunchKernelGGL((llm_qkv_rope_stream_kernel<WT, CH, false>), sgrid, dim3(256), 0, stream, X, gamma, eps,               \
                               static_cast<const WT*>(W), bias, n_heads, n_kv_heads, head_dim, cos_t, sin_t, Q, Kc, Vc, pos, pos_ptr, \
                               nullptr, nullptr, 0, nullptr);                                                                        \
    } while (0)
        if (bf16) {
            if (k == 2048) KJ_QKVS(uint16_t, 4);
            else if (k == 4096) KJ_QKVS(uint16_t, 8);
            else KJ_QKVS(uint16_t, 16);
        } else {
            if (k == 2048) KJ_QKVS(float, 4);
            else if (k == 4096) KJ_QKVS(float, 8);
            else KJ_QKVS(float, 16);
        }
#undef KJ_QKVS
        return hipGetLastError();
    }
    const dim3 grid((unsigned)rt.workgroups);
    const int chunks = rt.ch;
#define KJ_QKV(WT, CH)                                                                                                              \
    hipLaunchKernelGGL((llm_qkv_rope_kernel<WT, CH>), grid, dim3(256), 0, stream, X, gamma, eps, static_cast<const WT*>(W), bias, k, \
                       n_heads, n_kv_heads, head_dim, cos_t, sin_t, Q, Kc, Vc, pos, pos_ptr)
    if (bf16) {
        if (chunks <= 1) KJ_QKV(uint16_t, 1);
        else if (chunks <= 2) KJ_QKV(uint16_t, 2);
        else KJ_QKV(uint16_t, 4);
    } else {
        if (chunks <= 1) KJ_QKV(float, 1);
        else if (chunks <= 2) KJ_QKV(float, 2);
        else KJ_QKV(float, 4);
    }
#undef KJ_QKV
    return hipGetLastError();
}

bool llm_gemv_streams(int k, const void* W, const void* W2)
{
    return (k == 2048 || k == 4096 || k == 8192) && (reinterpret_cast<uintptr_t>(W) & 15) == 0 && (!W2 || (reinterpret_cast<uintptr_t>(W2) & 15) == 0);
}

bool llm_gemv_merges_attention(int k, int splits, int head_dim)
{
    if (head_dim < 4 || (head_dim & 3) || k % head_dim) return false;
    return (k == 2048 && splits >= 1 && splits <= 8) || (k == 4096 && splits >= 1 && splits <= 4);
}

hipError_t launch_llm_gemv(const LlmGemvArgs& a, hipStream_t stream)
{
    // (slabs are merged by the weight-streaming kernel alone: any other size would read them as a context row)
    if (a.att_splits > 0 && (a.rows != 1 || a.seg_q != 0 || !a.R || !llm_gemv_merges_attention(a.k, a.att_splits, a.att_head_dim)))
        return hipErrorInvalidValue;
    if (a.norm_out && !(a.rows == 1 && a.seg_q == 0 && a.gamma && llm_gemv_streams(a.k, a.W, a.W2))) return hipErrorInvalidValue;
    // LayerNorm needs gamma and beta and takes no residual / SwiGLU epilogue; GELU-tanh comes only after LayerNorm (GPT-2's c_fc)
    if (a.layernorm && (!a.gamma || !a.beta || a.R || a.swiglu || a.att_splits > 0 || a.norm_out)) return hipErrorInvalidValue;
    if (a.gelu_tanh && (!a.layernorm || a.seg_q != 0)) return hipErrorInvalidValue;
    // SwiGLU comes only after RMSNorm, a residual only without a norm (the pairs at launch_gemv_t)
    if ((a.swiglu && (!a.gamma || a.R)) || (a.R && a.gamma)) return hipErrorInvalidValue;
    if (a.rows <= 0 || a.n_out <= 0) return hipSuccess;
    if (a.rows > LLM_MAX_ROWS || (a.k & 7) || (a.ldx & 3) || (reinterpret_cast<uintptr_t>(a.X) & 15) ||
        (reinterpret_cast<uintptr_t>(a.W) & 15))
        return hipErrorInvalidValue;
    return a.bf16 ? launch_gemv_t<uint16_t>(a, stream) : launch_gemv_t<float>(a, stream);
}

hipError_t launch_rope(float* x, int64_t ldx, int rows, int n_heads, int head_dim, const float* cos_t, const float* sin_t, int pos,
                       const int* pos_ptr, int at_cache_row, hipStream_t stream)
{
    const int total = rows * n_heads * (head_dim / 2);
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(rope_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, ldx, rows, n_heads, head_dim, cos_t,
                       sin_t, pos, pos_ptr, at_cache_row);
    return hipGetLastError();
}

hipError_t launch_rmsnorm(const float* x, const float* gamma, float eps, int rows, int hidden, float* out, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if ((hidden & 3) == 0) {  // one workgroup per row, 16-byte loads (the wave-per-row kernel with scalar loads: 16 vs 5 us at 128 rows)
        hipLaunchKernelGGL(rmsnorm_block_kernel, dim3((unsigned)rows), dim3(256), 0, stream, x, gamma, eps, hidden, out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(rmsnorm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, gamma, eps, rows, hidden, out);
    return hipGetLastError();
}

hipError_t launch_llm_embed(const uint32_t* ids, int n, int hidden, int vocab, const void* table, int bf16, float* out,
                            hipStream_t stream)
{
    if (hidden & 7) return hipErrorInvalidValue;
    if (bf16)
        hipLaunchKernelGGL(llm_embed_kernel<uint16_t>, dim3((unsigned)n), dim3(256), 0, stream, ids, hidden, vocab,
                           static_cast<const uint16_t*>(table), out);
    else
        hipLaunchKernelGGL(llm_embed_kernel<float>, dim3((unsigned)n), dim3(256), 0, stream, ids, hidden, vocab,
                           static_cast<const float*>(table), out);
    return hipGetLastError();
}

namespace {

// GPT-2 embeddings (gpt2/cpu_decoder.rs:371-376): row s = wte[ids[s]] + wpe[p + s], p = *pos_ptr or pos (an id >= vocab
// or a position >= max_pos leaves that part zero).  ROW_POS (lanes: independent sequences): row s sits at row_pos[s].
template <typename WT, bool ROW_POS>
__global__ __launch_bounds__(256) void llm_embed_pos_kernel(const uint32_t* __restrict__ ids, int hidden, int vocab,
                                                            const WT* __restrict__ table, const WT* __restrict__ pos_table, int max_pos,
                                                            int pos, const int* __restrict__ pos_ptr, float* __restrict__ out,
                                                            const int* __restrict__ row_pos)
{
    const int s = blockIdx.x;
    const uint32_t id = ids[s];
    const int p = ROW_POS ? row_pos[s] : (pos_ptr ? *pos_ptr : pos) + s;
    for (int i = threadIdx.x; i < hidden / 8; i += 256) {
        F8 v, w;
#pragma unroll
        for (int c = 0; c < 8; ++c) v.v[c] = w.v[c] = 0.0f;
        if (id < (uint32_t)vocab) v = load8(table + (int64_t)id * hidden, i);
        if (p >= 0 && p < max_pos) w = load8(pos_table + (int64_t)p * hidden, i);
        f32x4 a, b;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = v.v[c] + w.v[c];
            b[c] = v.v[4 + c] + w.v[4 + c];
        }
        *reinterpret_cast<f32x4*>(out + (int64_t)s * hidden + i * 8) = a;
        *reinterpret_cast<f32x4*>(out + (int64_t)s * hidden + i * 8 + 4) = b;
    }
}

__global__ __launch_bounds__(256) void gelu_tanh_kernel(float* __restrict__ x, size_t n4)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 v = reinterpret_cast<f32x4*>(x)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = gelu_tanh(v[c]);
        reinterpret_cast<f32x4*>(x)[i] = v;
    }
}

}  // namespace

hipError_t launch_llm_embed_pos(const uint32_t* ids, int n, int hidden, int vocab, const void* table, const void* pos_table, int max_pos,
                                int bf16, int pos, const int* pos_ptr, float* out, hipStream_t stream, const int* row_pos)
{
    if (hidden & 7) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
#define KJ_EP(WT, ROW_POS)                                                                                                          \
    hipLaunchKernelGGL((llm_embed_pos_kernel<WT, ROW_POS>), dim3((unsigned)n), dim3(256), 0, stream, ids, hidden, vocab,            \
                       static_cast<const WT*>(table), static_cast<const WT*>(pos_table), max_pos, pos, pos_ptr, out, row_pos)
    if (bf16 && row_pos) KJ_EP(uint16_t, true);
    else if (bf16) KJ_EP(uint16_t, false);
    else if (row_pos) KJ_EP(float, true);
    else KJ_EP(float, false);
#undef KJ_EP
    return hipGetLastError();
}

hipError_t launch_gelu_tanh(float* x, size_t n, hipStream_t stream)
{
    if (n % 4 || (reinterpret_cast<uintptr_t>(x) & 15)) return hipErrorInvalidValue;
    const size_t n4 = n / 4;
    if (n4 == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(gelu_tanh_kernel, dim3(grid), dim3(256), 0, stream, x, n4);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampled decoding: what of sample_token (common/sampling.rs:81-114) and of the logits processors (:8-57) is O(vocab) runs
// here, on the logits where the vocabulary head left them; the host gets a few hundred (token, logit) pairs instead of
// 4 x vocab bytes and finishes the filters on them exactly (sampling.cpp, sampling_distribution_candidates).
//
//   logits processors: repetition penalty once per occurrence of every past token (counts per token + the list of distinct
//     tokens are kept on the device, updated by one tiny kernel per new token); no-repeat-n-gram bans by one thread per
//     window of the history.
//   sample_max:     per-workgroup maxima (the first launch also clears the histogram of the previous token);
//   sample_hist:    m = max; histogram of (m - logit) in bins of 1/8 (count and exp mass per bin); per-workgroup sums of
//                   exp(logit - m), each in a fixed order (the total is deterministic, but not the reference's index order:
//                   the host treats it as such);
//   sample_compact: every workgroup derives the cut `tau` from the histogram -- the distance below the maximum that holds
//                   top_k tokens and top_p of the mass, two bins of margin, and ln(1 / min_p) when min_p filters the whole
//                   vocabulary -- then appends every token with logit >= m - tau to the candidate list.
// A list longer than its capacity, or a cut the histogram cannot place, is reported in the header and the host falls back
// to fetching the logits.
// The three cut kernels take the row from blockIdx.y: row r of logits [., ld] has scratch[r], headers[r] and its own `cap`
// candidate slots.  The same SAMPLE_BLOCKS workgroups walk a row in the same order whatever the row count, and the per-workgroup
// maxima and sums are combined in a fixed order, so a row's mx and sum do not depend on the launcher.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SAMPLE_BLOCKS = 64, SAMPLE_BINS = 512;

struct SampleScratch {                 // device memory, zero-initialised once
    float part_max[SAMPLE_BLOCKS];
    float part_sum[SAMPLE_BLOCKS];
    unsigned hist_count[SAMPLE_BINS + 1];
    float hist_mass[SAMPLE_BINS + 1];
};

__global__ __launch_bounds__(256) void sample_max_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                         SampleScratch* __restrict__ scratch, SampleHeader* __restrict__ headers)
{
    __shared__ float red[4];
    const float* row = logits + (int64_t)blockIdx.y * ld;
    SampleScratch* sc = scratch + blockIdx.y;
    float m = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) m = fmaxf(m, row[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) sc->part_max[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    // (the histogram and the candidate counter of the previous token are dead by now)
    for (int b = blockIdx.x * 256 + threadIdx.x; b <= SAMPLE_BINS; b += gridDim.x * 256) {
        sc->hist_count[b] = 0u;
        sc->hist_mass[b] = 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        headers[blockIdx.y].count = 0u;
        headers[blockIdx.y].overflow = 0u;
    }
}

__global__ __launch_bounds__(256) void sample_hist_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                          SampleScratch* __restrict__ scratch)
{
    __shared__ unsigned h_count[SAMPLE_BINS + 1];
    __shared__ float h_mass[SAMPLE_BINS + 1];
    __shared__ float red[4];
    const float* row = logits + (int64_t)blockIdx.y * ld;
    SampleScratch* sc = scratch + blockIdx.y;
    for (int b = threadIdx.x; b <= SAMPLE_BINS; b += 256) {
        h_count[b] = 0u;
        h_mass[b] = 0.0f;
    }
    float m = -INFINITY;
    for (int b = 0; b < SAMPLE_BLOCKS; ++b) m = fmaxf(m, sc->part_max[b]);
    __syncthreads();
    float sum = 0.0f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < vocab; i += gridDim.x * 256) {
        const float v = row[i];
        const float e = expf(v - m);
        const float d = (m - v) * 8.0f;
        const int bin = d < (float)SAMPLE_BINS ? (int)d : SAMPLE_BINS;  // (NaN and -inf land in the last bin)
        sum += e;
        atomicAdd(&h_count[bin], 1u);
        atomicAdd(&h_mass[bin], e);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) sc->part_sum[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    for (int b = threadIdx.x; b <= SAMPLE_BINS; b += 256) {
        if (h_count[b]) {
            atomicAdd(&sc->hist_count[b], h_count[b]);
            atomicAdd(&sc->hist_mass[b], h_mass[b]);
        }
    }
}

// The cut of one row from its scratch: m = the maximum, sum = the per-workgroup sums in their fixed order, tau = how far below
// the maximum the candidates reach -- enough tokens for top-k, enough mass for top-p (the histogram's masses are summed in no
// fixed order: a relative margin on top of the two bins), everything min-p can keep when it filters the whole vocabulary.
// Returns whether no usable cut exists.
__device__ __forceinline__ bool sample_cut(const SampleScratch* __restrict__ sc, int vocab, long long top_k, float top_p, float min_p,
                                           float& m, float& sum, float& tau)
{
    m = -INFINITY;
    sum = 0.0f;
    for (int b = 0; b < SAMPLE_BLOCKS; ++b) m = fmaxf(m, sc->part_max[b]);
    for (int b = 0; b < SAMPLE_BLOCKS; ++b) sum += sc->part_sum[b];
    const bool k_on = top_k >= 0 && top_k < (long long)vocab;  // (top_k >= vocab filters nothing)
    const double need_count = k_on ? (double)top_k : 1.0;
    const double need_mass = top_p >= 0.0f ? (double)top_p * (double)sum * 1.001 : 0.0;
    double cnt = 0.0, mass = 0.0;
    tau = INFINITY;
    for (int b = 0; b < SAMPLE_BINS; ++b) {
        cnt += (double)sc->hist_count[b];
        mass += (double)sc->hist_mass[b];
        if (cnt >= need_count && mass > need_mass) {
            tau = (float)(b + 2) / 8.0f;
            break;
        }
    }
    const bool minp_on_all = min_p >= 0.0f && !k_on && !(top_p >= 0.0f && top_p < 1.0f);
    if (minp_on_all) tau = min_p > 0.0f ? fmaxf(tau, -logf(min_p) + 0.25f) : INFINITY;
    return !(tau < 1e30f) || !(m > -INFINITY) || !(m < INFINITY);
}

// chunked: slot s of the row is entry sample_rows_slot(row, s) of `candidates` (launch_sample_candidates_rows), else entry s
// (launch_sample_candidates: one row, a contiguous list).
__global__ __launch_bounds__(256) void sample_compact_kernel(const float* __restrict__ logits, int64_t ld, int vocab, long long top_k,
                                                             float top_p, float min_p, const SampleScratch* __restrict__ scratch,
                                                             SampleHeader* __restrict__ headers, SampleCandidate* __restrict__ candidates,
                                                             int cap, bool chunked)
{
    __shared__ float s_floor;
    __shared__ int s_all;
    const float* row = logits + (int64_t)blockIdx.y * ld;
    const SampleScratch* sc = scratch + blockIdx.y;
    SampleHeader* header = headers + blockIdx.y;
    if (threadIdx.x == 0) {  // the cut, from this row's histogram
        float m, sum, tau;
        s_all = sample_cut(sc, vocab, top_k, top_p, min_p, m, sum, tau);
        s_floor = m - tau;
        if (blockIdx.x == 0) {
            header->mx = m;
            header->sum = sum;
            header->floor = s_all ? -INFINITY : m - tau;
        }
    }
    __syncthreads();
    if (s_all) {  // no usable cut: the host takes the logits (floor = -inf: every token is above it, none is appended)
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            header->count = (uint32_t)vocab;
            header->overflow = 1u;
        }
        return;
    }
    const float floor = s_floor;
    const int lane = threadIdx.x & 63;
    for (int i0 = blockIdx.x * 256; i0 < vocab; i0 += gridDim.x * 256) {
        const int i = i0 + threadIdx.x;
        const float v = i < vocab ? row[i] : -INFINITY;
        const bool keep = i < vocab && v >= floor;
        const unsigned long long bits = __ballot(keep);
        if (bits == 0ull) continue;
        unsigned base = 0u;
        if (lane == 0) base = atomicAdd(&header->count, (unsigned)__popcll(bits));
        base = __shfl(base, 0, kWave);
        if (keep) {
            const unsigned slot = base + (unsigned)__popcll(bits & ((1ull << lane) - 1ull));
            if (slot < (unsigned)cap) candidates[chunked ? sample_rows_slot((int)blockIdx.y, (int)slot) : slot] = SampleCandidate{(uint32_t)i, v};
            else header->overflow = 1u;
        }
    }
}

// counts[t] += 1 for each of the n tokens; a token seen for the first time joins the list of distinct tokens
__global__ __launch_bounds__(256) void token_counts_kernel(const int32_t* __restrict__ tokens, int n, int vocab, int* __restrict__ counts,
                                                           int32_t* __restrict__ distinct, int* __restrict__ n_distinct)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = tokens[i];
    if (t < 0 || t >= vocab) return;
    if (atomicAdd(&counts[t], 1) == 0) distinct[atomicAdd(n_distinct, 1)] = t;
}

// apply_repetition_penalty (sampling.rs:8-27 / generator.rs:331-337): s < 0 ? s * penalty : s / penalty, once per OCCURRENCE
// of the token in the history, in sequence (each application rounds).
// Row r = blockIdx.y of a verify block predicts the token after ids[0..r]: its history is the counted one (up to and including
// ids[0]) plus ids[1..r].  One thread per distinct token of the counted history, then one per draft position of the row: a draft
// token the counted history does not hold is handled by the thread of its first occurrence in ids[1..r].  Row 0 never reads
// ids: launch_logits_processors is the grid of one row with ids == nullptr.
__global__ __launch_bounds__(256) void repetition_penalty_kernel(float* __restrict__ logits, int64_t ld, int vocab, const uint32_t* __restrict__ ids,
                                                                 const int* __restrict__ counts, const int32_t* __restrict__ distinct,
                                                                 const int* __restrict__ n_distinct, float penalty)
{
    const int r = blockIdx.y;
    float* row = logits + (int64_t)r * ld;
    const int nd = *n_distinct;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < nd + r; j += gridDim.x * 256) {
        int t, c;
        if (j < nd) {
            t = distinct[j];
            if (t < 0 || t >= vocab) continue;
            c = counts[t];
        } else {
            const int i = j - nd + 1;
            if (ids[i] >= (uint32_t)vocab) continue;
            t = (int)ids[i];
            if (counts[t] != 0) continue;  // (in `distinct`: the thread above has it)
            bool first = true;
            for (int q = 1; q < i; ++q) first = first && ids[q] != ids[i];
            if (!first) continue;
            c = 0;
        }
        for (int q = 1; q <= r; ++q) c += ids[q] == (uint32_t)t ? 1 : 0;
        float s = row[t];
        for (; c > 0; --c) s = s < 0.0f ? __fmul_rn(s, penalty) : __fdiv_rn(s, penalty);
        row[t] = s;
    }
}

// apply_no_repeat_ngram (sampling.rs:29-57): every window of the history whose first n - 1 tokens equal the last n - 1 bans
// its n-th token
__global__ __launch_bounds__(256) void no_repeat_ngram_kernel(float* __restrict__ logits, int vocab, const int32_t* __restrict__ tokens,
                                                              int len, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i + n > len) return;
    const int32_t* tail = tokens + len - (n - 1);
    for (int k = 0; k < n - 1; ++k)
        if (tokens[i + k] != tail[k]) return;
    const int banned = tokens[i + n - 1];
    if (banned >= 0 && banned < vocab) logits[banned] = -INFINITY;
}

hipError_t launch_argmax(const float* logits, int vocab, unsigned long long* best_scratch, int32_t* out, int32_t* history, int* count,
                         int* pos, hipStream_t stream)
{
    int blocks = (vocab + 2047) / 2048;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(argmax_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, logits, (int64_t)0, vocab, 0,
                       static_cast<const int*>(nullptr), best_scratch);
    hipLaunchKernelGGL(argmax_finalize_kernel, dim3(1), dim3(1), 0, stream, best_scratch, out, history, count, pos);
    return hipGetLastError();
}


size_t sample_scratch_bytes() { return sizeof(SampleScratch); }

// The cut of `rows` rows: SAMPLE_BLOCKS workgroups per row, whatever the row count, so a row's walk order does not depend on it.
static hipError_t launch_sample_cut(const float* logits, int64_t ld, int rows, int vocab, int64_t top_k, float top_p, float min_p,
                                    void* scratch, SampleHeader* headers, SampleCandidate* candidates, int capacity, bool chunked,
                                    hipStream_t stream)
{
    SampleScratch* sc = static_cast<SampleScratch*>(scratch);
    const dim3 grid(SAMPLE_BLOCKS, (unsigned)rows);
    hipLaunchKernelGGL(sample_max_kernel, grid, dim3(256), 0, stream, logits, ld, vocab, sc, headers);
    hipLaunchKernelGGL(sample_hist_kernel, grid, dim3(256), 0, stream, logits, ld, vocab, sc);
    hipLaunchKernelGGL(sample_compact_kernel, grid, dim3(256), 0, stream, logits, ld, vocab, (long long)top_k, top_p, min_p, sc, headers,
                       candidates, capacity, chunked);
    return hipGetLastError();
}

hipError_t launch_sample_candidates(const float* logits, int vocab, int64_t top_k, float top_p, float min_p, void* scratch,
                                    SampleHeader* header, SampleCandidate* candidates, int capacity, hipStream_t stream)
{
    return launch_sample_cut(logits, 0, 1, vocab, top_k, top_p, min_p, scratch, header, candidates, capacity, false, stream);
}

hipError_t launch_token_counts(const int32_t* tokens, int n, int vocab, int* counts, int32_t* distinct, int* n_distinct, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(token_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tokens, n, vocab, counts, distinct,
                       n_distinct);
    return hipGetLastError();
}

hipError_t launch_logits_processors(float* logits, int vocab, const int32_t* tokens, int len, const int* counts, const int32_t* distinct,
                                    const int* n_distinct, float repetition_penalty, int no_repeat_ngram, hipStream_t stream)
{
    if (repetition_penalty != 1.0f && len > 0)
        hipLaunchKernelGGL(repetition_penalty_kernel, dim3((unsigned)((std::min(len, vocab) + 255) / 256)), dim3(256), 0, stream, logits,
                           (int64_t)0, vocab, static_cast<const uint32_t*>(nullptr), counts, distinct, n_distinct, repetition_penalty);
    if (no_repeat_ngram > 0 && len + 1 >= no_repeat_ngram && len >= no_repeat_ngram)
        hipLaunchKernelGGL(no_repeat_ngram_kernel, dim3((unsigned)((len - no_repeat_ngram + 1 + 255) / 256)), dim3(256), 0, stream, logits,
                           vocab, tokens, len, no_repeat_ngram);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------------------------------
// Lanes: up to 8 independent sequences decoded in lock step (llm.cpp: LlmModel::lane_step).
namespace {

// Multi-row weight-streaming GEMV: Y[r, n] = epi(norm?(X[r, :]) . W[n, :] + bias[n]) for 2..8 INDEPENDENT rows, the design of
// llm_gemv_stream_kernel with every 16-byte weight piece multiplied into all resident rows.
//
// LDS scheme (160 KB per CU): the workgroup holds a K-SLICE of every row, [rows][SLICE] f32 with SLICE = CH * 512 (CH = 4:
// 2 048 columns, 64 KB at 8 rows, two workgroups per CU; CH = 2 serves K = 768 / 3 072 without padded pieces).  K <= SLICE
// (the Q|K|V, gate/up, c_fc and vocabulary-head stages): the rows are normalised ONCE per workgroup into LDS and the
// workgroup loops over its batches of columns.  K > SLICE (down projection, K = 8 192 / 14 336; K = 3 072): the slices are
// staged one after the other and the accumulators of the workgroup's columns stay in registers across them; the grid then
// covers the columns, so every slice is staged once per workgroup.  Row statistics (RMSNorm / LayerNorm) are taken over the
// whole row before the first slice: one wave per row.
// Per (batch, slice) a wave owns CPW columns: CPW x CH (x 2 for f32, x 2 for the SwiGLU pair) non-temporal 16-byte loads
// per lane, 16 with WIDE, all issued before the first FMA; the slice of the input rows for the next stage is requested
// BEFORE those weights (the counter retires in order: x must not wait behind the weights) and written to LDS after.  The
// inner loop is FMAs only: acc[column][row] = fmaf(x, widen(w), acc) -- the arithmetic of llm_gemv_kernel, summed in a
// different order.  A piece past the end of K reads piece 0 again and meets zeros in LDS.
constexpr int lanes_cols_per_wave(int ch, int lpp, int nm, bool wide)
{
    return !wide ? 1 : (16 / (ch * lpp * nm) < 1 ? 1 : (16 / (ch * lpp * nm) > 4 ? 4 : 16 / (ch * lpp * nm)));
}

template <typename WT, int EPI, int NORM, int CH, bool WIDE>
__global__ __launch_bounds__(256) void llm_gemv_lanes_kernel(const float* __restrict__ X, int64_t ldx, int rows,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             const WT* __restrict__ W, const WT* __restrict__ W2,
                                                             const float* __restrict__ bias, const float* R, int64_t ldr, int n_out,
                                                             int k, int seg_q, int seg_kv, float* Y0, int64_t ldy0, float* Y1, float* Y2,
                                                             int64_t ldy12, int row_off, const int* __restrict__ row_off_ptr)
{
    constexpr bool BF16 = sizeof(WT) == 2;
    constexpr int NM = EPI == LE_SWIGLU ? 2 : 1;
    constexpr int LPP = BF16 ? 1 : 2;
    constexpr int CPW = lanes_cols_per_wave(CH, LPP, NM, WIDE);
    constexpr int SLICE = CH * 512;
    constexpr int XV = CH / 2;  // f32x4 pieces of one row's slice per thread
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float lanes_xs[];  // [rows][SLICE]
    __shared__ float st_mu[LLM_MAX_ROWS], st_sc[LLM_MAX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = (k + SLICE - 1) / SLICE;
    const int nbatches = (n_out + 4 * CPW - 1) / (4 * CPW);

    f32x4 xv[LLM_MAX_ROWS][XV], gv[XV], bv[XV];
    auto load_x = [&](int s) {
#pragma unroll
        for (int j = 0; j < XV; ++j) {
            const int col = s * SLICE + (tid + j * 256) * 4;
            const bool in = col < k;
            gv[j] = (NORM != NK_NONE && in) ? *reinterpret_cast<const f32x4*>(gamma + col) : f32x4{0.f, 0.f, 0.f, 0.f};
            bv[j] = (NORM == NK_LN && in) ? *reinterpret_cast<const f32x4*>(beta + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < LLM_MAX_ROWS; ++r)
                xv[r][j] = (r < rows && in) ? *reinterpret_cast<const f32x4*>(X + r * ldx + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int r = 0; r < LLM_MAX_ROWS; ++r) {
            if (r < rows) {
#pragma unroll
                for (int j = 0; j < XV; ++j) {
                    f32x4 v = xv[r][j];
                    if (NORM == NK_RMS) {
                        const float rms = st_sc[r];
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = (v[c] / rms) * gv[j][c];
                    }
                    if (NORM == NK_LN) {
                        const float mu = st_mu[r], inv = st_sc[r];
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = (v[c] - mu) * inv * gv[j][c] + bv[j][c];  // (past K: gamma = beta = 0)
                    }
                    *reinterpret_cast<f32x4*>(lanes_xs + r * SLICE + (tid + j * 256) * 4) = v;
                }
            }
        }
    };
    u32x4 raw[NM][CPW][CH][LPP];
    auto issue = [&](int nb, int s) {
        const int n0 = (nb * 4 + wave) * CPW;
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int cc = 0; cc < CPW; ++cc) {
                const int n = n0 + cc < n_out ? n0 + cc : n_out - 1;
                const char* row = reinterpret_cast<const char*>((m == 0 ? W : W2) + (int64_t)n * k);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    int e = s * SLICE + (c * 64 + lane) * 8;
                    e = e < k ? e : 0;
#pragma unroll
                    for (int l = 0; l < LPP; ++l) raw[m][cc][c][l] = load_nt16(row + (size_t)e * sizeof(WT) + l * 16);
                }
            }
    };

    int nb = blockIdx.x, s = 0;
    load_x(0);
    issue(nb, 0);
    // row statistics over the whole row, one wave per row (the loads above are in flight meanwhile)
    if (NORM != NK_NONE) {
        const int k8 = k >> 3;
        for (int r = wave; r < rows; r += 4) {
            const float* xr = X + r * ldx;
            float mu = 0.0f, sc;
            if (NORM == NK_RMS) {
                float a = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(xr, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) a = fmaf(x.v[c], x.v[c], a);
                }
                sc = sqrtf(wave_sum(a) / (float)k + eps);  // the rms; the reference divides by it
            } else {
                float a = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(xr, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) a += x.v[c];
                }
                mu = wave_sum(a) / (float)k;
                float v = 0.0f;
                for (int i = lane; i < k8; i += 64) {
                    const F8 x = load8(xr, i);
#pragma unroll
                    for (int c = 0; c < 8; ++c) v = fmaf(x.v[c] - mu, x.v[c] - mu, v);
                }
                sc = 1.0f / sqrtf(wave_sum(v) / (float)k + eps);  // the inverse standard deviation
            }
            if (lane == 0) {
                st_mu[r] = mu;
                st_sc[r] = sc;
            }
        }
        __syncthreads();
    }

    float acc[NM][CPW][LLM_MAX_ROWS];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int cc = 0; cc < CPW; ++cc)
#pragma unroll
            for (int r = 0; r < LLM_MAX_ROWS; ++r) acc[m][cc][r] = 0.0f;
    bool first = true;
    for (;;) {
        if (first || ns > 1) {
            if (!first) __syncthreads();  // every wave is done with the slice in LDS
            store_x();
            __syncthreads();
        }
        first = false;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int r = 0; r < LLM_MAX_ROWS; ++r) {
                if (r < rows) {
                    const f32x4 xa = *reinterpret_cast<const f32x4*>(lanes_xs + r * SLICE + (c * 64 + lane) * 8);
                    const f32x4 xb = *reinterpret_cast<const f32x4*>(lanes_xs + r * SLICE + (c * 64 + lane) * 8 + 4);
#pragma unroll
                    for (int m = 0; m < NM; ++m)
#pragma unroll
                        for (int cc = 0; cc < CPW; ++cc) {
                            if (BF16) {
                                acc[m][cc][r] = dot8_bf16(raw[m][cc][c][0], xa, xb, acc[m][cc][r]);
                            } else {
                                const f32x4 wa = __builtin_bit_cast(f32x4, raw[m][cc][c][0]);
                                const f32x4 wb = __builtin_bit_cast(f32x4, raw[m][cc][c][LPP - 1]);
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[m][cc][r] = fmaf(xa[e], wa[e], acc[m][cc][r]);
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[m][cc][r] = fmaf(xb[e], wb[e], acc[m][cc][r]);
                            }
                        }
                }
            }
        }
        // the next (batch, slice): its rows' slice, then its weights, requested before this batch's cross-lane sums and stores
        int s2 = s + 1, nb2 = nb;
        if (s2 == ns) {
            s2 = 0;
            nb2 = nb + (int)gridDim.x;
        }
        const bool more = nb2 < nbatches;
        if (more) {
            if (ns > 1) load_x(s2);
            issue(nb2, s2);
        }
        if (s == ns - 1) {
            const int n0 = (nb * 4 + wave) * CPW;
#pragma unroll
            for (int cc = 0; cc < CPW; ++cc) {
                float mine = 0.0f, mine2 = 0.0f;  // lane r keeps row r's sum
#pragma unroll
                for (int r = 0; r < LLM_MAX_ROWS; ++r) {
                    if (r < rows) {
                        const float t = wave_sum(acc[0][cc][r]);
                        mine = lane == r ? t : mine;
                        if (EPI == LE_SWIGLU) {
                            const float t2 = wave_sum(acc[NM - 1][cc][r]);
                            mine2 = lane == r ? t2 : mine2;
                        }
                    }
#pragma unroll
                    for (int m = 0; m < NM; ++m) acc[m][cc][r] = 0.0f;
                }
                const int n = n0 + cc;
                if (lane < rows && n < n_out) {
                    float v = mine + (bias ? bias[n] : 0.0f);
                    if (EPI == LE_SWIGLU) v = (v / (1.0f + expf(-v))) * mine2;  // silu(gate) * up
                    if (EPI == LE_GELU_TANH) v = gelu_tanh(v);
                    if (EPI == LE_RESIDUAL) v += R[lane * ldr + n];
                    int which = 0;
                    int64_t col = n;
                    if (seg_q > 0 && n >= seg_q) {
                        which = 1 + (n - seg_q) / seg_kv;
                        col = (n - seg_q) - (int64_t)(which - 1) * seg_kv;
                    }
                    float* Y = which == 0 ? Y0 : (which == 1 ? Y1 : Y2);
                    const int64_t ldy = which == 0 ? ldy0 : ldy12;
                    const int64_t r0 = which == 0 ? 0 : (row_off_ptr ? *row_off_ptr : row_off);
                    Y[(r0 + lane) * ldy + col] = v;
                }
            }
        }
        if (!more) break;
        s = s2;
        nb = nb2;
    }
}

// Lane rotate-and-scatter: row `lane` of the staging buffer [lanes, H + 2 kv] holds Q | K | V of that lane's new token at
// position pos[lane].  Q is rotated in place (rope/mod.rs:156-176, pairs (i, i + d/2)), K is rotated into row pos[lane] of the
// lane's cache and V copied there; rotate == 0 (GPT-2): K and V are copied.  A lane that is not live, or whose position is
// not a row of its cache (a lane stopped at its context limit has pos == capacity), writes nothing.
__global__ __launch_bounds__(256) void lane_rope_scatter_kernel(float* __restrict__ qkv, int64_t ld, int n_heads, int n_kv_heads,
                                                                int head_dim, const float* __restrict__ cos_t,
                                                                const float* __restrict__ sin_t, float* __restrict__ Kc,
                                                                float* __restrict__ Vc, int64_t lane_stride, int capacity,
                                                                const int* __restrict__ pos, const int* __restrict__ live, int rotate)
{
    const int lane = blockIdx.x;
    if (!live[lane]) return;
    const int p = pos[lane];
    if (p < 0 || p >= capacity) return;
    const int half = head_dim >> 1, H = n_heads * head_dim, kv = n_kv_heads * head_dim;
    float* row = qkv + (int64_t)lane * ld;
    float* kdst = Kc + (int64_t)lane * lane_stride + (int64_t)p * kv;
    float* vdst = Vc + (int64_t)lane * lane_stride + (int64_t)p * kv;
    if (rotate) {
        for (int idx = threadIdx.x; idx < (n_heads + n_kv_heads) * half; idx += 256) {
            const int i = idx % half, h = idx / half;
            const float c = cos_t[(int64_t)p * half + i], s = sin_t[(int64_t)p * half + i];
            const bool is_q = h < n_heads;
            const float* src = is_q ? row + h * head_dim : row + H + (h - n_heads) * head_dim;
            float* dst = is_q ? row + h * head_dim : kdst + (h - n_heads) * head_dim;
            const float x0 = src[i], x1 = src[i + half];
            dst[i] = x0 * c - x1 * s;
            dst[i + half] = x0 * s + x1 * c;
        }
    } else {
        for (int i = threadIdx.x; i < kv; i += 256) kdst[i] = row[H + i];
    }
    for (int i = threadIdx.x; i < kv; i += 256) vdst[i] = row[H + kv + i];
}

// The pick of a live lane: the token joins the lane's history, count (and, after a step, pos) advance; the lane stays live
// -- and the token becomes its next input -- unless the token is one of its stop ids, it has its max_new_tokens, or its
// cache is full.  One wave, a thread per lane of [first_lane, first_lane + lanes) of either layout; a lane past the layout, a
// count that is no history entry and stop ids past the list are not followed.
__global__ __launch_bounds__(kMaxWideLanes) void lane_pick_finalize_kernel(unsigned long long* __restrict__ best, LaneStateRef st,
                                                                           int32_t* __restrict__ history, int hist_stride, int first_lane,
                                                                           int lanes, int capacity, int advance)
{
    const int l = first_lane + threadIdx.x;
    if (l >= first_lane + lanes || l >= st.width || !st.live[l]) return;
    const int tok = (int)(uint32_t)(best[l] & 0xFFFFFFFFull);
    best[l] = 0ull;
    const int cnt = st.count[l];
    if (cnt >= 0 && cnt < hist_stride) history[(int64_t)l * hist_stride + cnt] = tok;
    st.count[l] = cnt + 1;
    if (advance) st.pos[l] += 1;
    bool stop = cnt + 1 >= st.limit[l] || st.pos[l] >= capacity;
    const int ns = min(st.n_stop[l], kMaxLaneStops);
    for (int e = 0; e < ns; ++e) stop = stop || st.stop[l][e] == tok;
    if (stop) st.live[l] = 0;
    else st.token[l] = tok;
}

}  // namespace

bool llm_gemv_lanes_takes(const LlmGemvArgs& a)
{
    return a.rows >= 1 && a.rows <= LLM_MAX_ROWS && a.k >= 512 && (a.k & 7) == 0 && (a.ldx & 3) == 0 && a.att_splits == 0 && !a.norm_out &&
           (reinterpret_cast<uintptr_t>(a.X) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.W) & 15) == 0 &&
           (!a.W2 || (reinterpret_cast<uintptr_t>(a.W2) & 15) == 0) && (!a.gamma || (reinterpret_cast<uintptr_t>(a.gamma) & 15) == 0) &&
           (!a.beta || (reinterpret_cast<uintptr_t>(a.beta) & 15) == 0);
}

LlmGemvLanesRoute llm_gemv_lanes_route(const LlmGemvArgs& a)
{
    LlmGemvLanesRoute r;
    r.taken = llm_gemv_lanes_takes(a) ? 1 : 0;
    if (!r.taken || a.n_out <= 0) return r;
    const int lpp = a.bf16 ? 1 : 2;
    // the slice width that pads K least (K = 768 / 3 072 -> 1 024, else 2 048)
    const int ch = ((a.k + 1023) / 1024) * 1024 - a.k < ((a.k + 2047) / 2048) * 2048 - a.k ? 2 : 4;
    const int nm = a.swiglu ? 2 : 1;
    const int ns = (a.k + ch * 512 - 1) / (ch * 512);
    // 16 loads per lane in flight where that still leaves two workgroups for every CU, else one column per wave
    const int cpw_wide = lanes_cols_per_wave(ch, lpp, nm, true);
    const bool wide = (a.n_out + 4 * cpw_wide - 1) / (4 * cpw_wide) >= 512;
    const int cpw = wide ? cpw_wide : 1;
    const int nbatches = (a.n_out + 4 * cpw - 1) / (4 * cpw);
    r.ch = ch;
    r.ns = ns;
    r.wide = wide ? 1 : 0;
    r.cpw = cpw;
    // one slice: the rows stay in LDS and the workgroup loops over its batches; several: the grid covers the columns
    r.workgroups = ns == 1 ? std::min(nbatches, 512) : nbatches;
    return r;
}

template <typename WT>
static hipError_t launch_gemv_lanes_t(const LlmGemvArgs& a, hipStream_t stream)
{
    const WT* W = static_cast<const WT*>(a.W);
    const WT* W2 = static_cast<const WT*>(a.W2);
    // (the slice width, the 16-load form and the grid are llm_gemv_lanes_route's)
    const LlmGemvLanesRoute rt = llm_gemv_lanes_route(a);
    const int ch = rt.ch, wgs = rt.workgroups;
    const bool wide = rt.wide != 0;
    const size_t lds = (size_t)a.rows * ch * 512 * sizeof(float);
#define KJ_LN3(EPI, NORM, CH, WIDE)                                                                                                  \
    do {                                                                                                                             \
        auto kern = llm_gemv_lanes_kernel<WT, EPI, NORM, CH, WIDE>;                                                                  \
        if (lds > 48 * 1024) {                                                                                                       \
            const hipError_t e = allow_dynamic_lds(kern, lds);                                                                       \
            if (e != hipSuccess) return e;                                                                                           \
        }                                                                                                                            \
        hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), lds, stream, a.X, a.ldx, a.rows, a.gamma, a.beta, a.eps, W, W2,     \
                           a.bias, a.R, a.ldr, a.n_out, a.k, a.seg_q, a.seg_kv, a.Y0, a.ldy0, a.Y1, a.Y2, a.ldy12, a.row_off,       \
                           a.row_off_ptr);                                                                                           \
    } while (0)
#define KJ_LN2(EPI, NORM)                                                                                                            \
    do {                                                                                                                             \
        if (ch == 2 && wide) KJ_LN3(EPI, NORM, 2, true);                                                                             \
        else if (ch == 2) KJ_LN3(EPI, NORM, 2, false);                                                                               \
        else if (wide) KJ_LN3(EPI, NORM, 4, true);                                                                                   \
        else KJ_LN3(EPI, NORM, 4, false);                                                                                            \
    } while (0)
    // the (epilogue, norm) pairs of launch_gemv_t
    if (a.layernorm) {
        if (a.gelu_tanh) KJ_LN2(LE_GELU_TANH, NK_LN);
        else KJ_LN2(LE_NONE, NK_LN);
    } else if (a.swiglu) KJ_LN2(LE_SWIGLU, NK_RMS);
    else if (a.R) KJ_LN2(LE_RESIDUAL, NK_NONE);
    else if (a.gamma) KJ_LN2(LE_NONE, NK_RMS);
    else KJ_LN2(LE_NONE, NK_NONE);
#undef KJ_LN2
#undef KJ_LN3
    return hipGetLastError();
}

hipError_t launch_llm_gemv_lanes(const LlmGemvArgs& a, hipStream_t stream, int* streamed)
{
    if (streamed) *streamed = 0;
    if (!llm_gemv_lanes_takes(a)) return launch_llm_gemv(a, stream);  // correct, but the rows are re-read for every column
    // the pairs launch_llm_gemv accepts
    if (a.layernorm && (!a.gamma || !a.beta || a.R || a.swiglu)) return hipErrorInvalidValue;
    if (a.gelu_tanh && (!a.layernorm || a.seg_q != 0)) return hipErrorInvalidValue;
    if ((a.swiglu && (!a.gamma || a.R || !a.W2)) || (a.R && a.gamma)) return hipErrorInvalidValue;
    if (a.n_out <= 0) return hipSuccess;
    if (streamed) *streamed = 1;
    return a.bf16 ? launch_gemv_lanes_t<uint16_t>(a, stream) : launch_gemv_lanes_t<float>(a, stream);
}

hipError_t launch_lane_rope_scatter(float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim, const float* cos_t,
                                    const float* sin_t, float* k_cache, float* v_cache, int64_t lane_stride, int capacity,
                                    LaneStateRef state, int rotate, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (lanes > state.width || (rotate && (head_dim & 1))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_rope_scatter_kernel, dim3((unsigned)lanes), dim3(256), 0, stream, qkv, ld, n_heads, n_kv_heads, head_dim, cos_t,
                       sin_t, k_cache, v_cache, lane_stride, capacity, state.pos, state.live, rotate);
    return hipGetLastError();
}

hipError_t launch_lane_pick(const float* logits, int64_t ld, int vocab, int lanes, int first_lane, unsigned long long* best_scratch,
                            LaneStateRef state, int32_t* history, int hist_stride, int capacity, int advance, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (first_lane < 0 || first_lane + lanes > state.width || vocab < 1 || hist_stride < 1) return hipErrorInvalidValue;
    int blocks = (vocab + 2047) / 2048;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(argmax_partial_kernel, dim3((unsigned)blocks, (unsigned)lanes), dim3(256), 0, stream, logits, ld, vocab, first_lane,
                       static_cast<const int*>(state.live), best_scratch);
    hipLaunchKernelGGL(lane_pick_finalize_kernel, dim3(1), dim3(kMaxWideLanes), 0, stream, best_scratch, state, history, hist_stride, first_lane,
                       lanes, capacity, advance);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Shared prompt prefix (llm.cpp: LlmModel::lane_copy_prefix): the first rows of the single-sequence cache into a lane's cache.
namespace {

// grid (x, 2 * layers): blockIdx.y picks the layer and K or V, the x blocks stride over the floats.  A pure stream: each
// thread moves 16 bytes per trip when both pointers allow it (uniform per block), 4 bytes otherwise and for the last
// count % 4 floats.  The words are moved as integers, so every bit pattern survives.  The pointers come out of the table, so
// the compiler cannot know that they are global memory: the address space is stated, for global instead of flat accesses.
typedef __attribute__((address_space(1))) const uint32_t gconst_u32;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 gconst_u4;
typedef __attribute__((address_space(1))) u32x4 g_u4;

__global__ __launch_bounds__(256) void kv_prefix_copy_kernel(const LlmKvCopyPair* __restrict__ table, int64_t dst_offset, int64_t count)
{
    const LlmKvCopyPair p = table[blockIdx.y >> 1];
    const bool v = (blockIdx.y & 1) != 0;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(v ? p.src_v : p.src_k);
    const uintptr_t da = reinterpret_cast<uintptr_t>((v ? p.dst_v : p.dst_k) + dst_offset);
    gconst_u32* __restrict__ src = reinterpret_cast<gconst_u32*>(sa);
    g_u32* __restrict__ dst = reinterpret_cast<g_u32*>(da);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    int64_t done = 0;
    if (((sa | da) & 15) == 0) {
        const int64_t n4 = count >> 2;
        gconst_u4* __restrict__ s4 = reinterpret_cast<gconst_u4*>(sa);
        g_u4* __restrict__ d4 = reinterpret_cast<g_u4*>(da);
        for (int64_t i = tid; i < n4; i += step) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (int64_t i = done + tid; i < count; i += step) dst[i] = src[i];
}

}  // namespace

hipError_t launch_kv_prefix_copy(const LlmKvCopyPair* table, int layers, int64_t dst_offset, int64_t count, hipStream_t stream)
{
    if (layers <= 0 || count <= 0) return hipSuccess;
    if (!table || dst_offset < 0 || layers > 32767) return hipErrorInvalidValue;
    int64_t blocks = (count / 4 + 255) / 256;  // one 16-byte trip per thread up to 256 blocks per cache, more trips beyond
    if (blocks < 1) blocks = 1;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(kv_prefix_copy_kernel, dim3((unsigned)blocks, (unsigned)(2 * layers)), dim3(256), 0, stream, table, dst_offset, count);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Qwen3: Q and K are RMS-normalised per head before the rotation.  One wave per (row, head); lane i < d/2 holds x[i] and
// x[i + d/2] (the lanes past d/2 hold zeros), so the sum of squares is one wave_sum, the rotation pairs sit in one lane, and
// there is no LDS and no barrier.  Arithmetic of rmsnorm_kernel ((x / sqrt(mean(x^2) + eps)) * gamma, rms_norm.rs:19-27), then
// of rope_kernel (rope/mod.rs:156-176).
namespace {

// One head in place at x, or from src into dst (the lane kernel's K): normalise, scale by gamma [d], rotate by table row p.
__device__ __forceinline__ void head_norm_rope(const float* src, float* dst, const float* __restrict__ gamma,
                                               float eps, const float* __restrict__ cos_t, const float* __restrict__ sin_t, int p,
                                               int head_dim, int lane)
{
    const int half = head_dim >> 1;
    const bool on = lane < half;
    const float x0 = on ? src[lane] : 0.0f, x1 = on ? src[lane + half] : 0.0f;
    float s = fmaf(x0, x0, 0.0f);
    s = fmaf(x1, x1, s);
    const float rms = sqrtf(wave_sum(s) / (float)head_dim + eps);  // every lane of the wave is here: the reduction is wave-wide
    if (!on) return;
    const float y0 = (x0 / rms) * gamma[lane], y1 = (x1 / rms) * gamma[lane + half];
    const float c = cos_t[(int64_t)p * half + lane], sn = sin_t[(int64_t)p * half + lane];
    dst[lane] = y0 * c - y1 * sn;
    dst[lane + half] = y0 * sn + y1 * c;
}

// rows x (n_heads + n_kv_heads) heads, four per workgroup.  Row r is at position p = (*pos_ptr | pos) + r; its Q heads are
// row r of q, its K heads row (k_at_cache_row ? p : r) of k.
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(float* __restrict__ q, int64_t ldq, float* __restrict__ k, int64_t ldk, int rows,
                                                           int n_heads, int n_kv_heads, int head_dim,
                                                           const float* __restrict__ gamma_q, const float* __restrict__ gamma_k, float eps,
                                                           const float* __restrict__ cos_t, const float* __restrict__ sin_t, int pos,
                                                           const int* __restrict__ pos_ptr, int k_at_cache_row)
{
    const int lane = threadIdx.x & 63;
    const int per_row = n_heads + n_kv_heads;
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);  // uniform over the wave
    if (job >= rows * per_row) return;
    const int r = job / per_row, h = job - r * per_row;
    const int p = (pos_ptr ? *pos_ptr : pos) + r;
    const bool is_q = h < n_heads;
    float* x = is_q ? q + (int64_t)r * ldq + h * head_dim : k + (int64_t)(k_at_cache_row ? p : r) * ldk + (h - n_heads) * head_dim;
    head_norm_rope(x, x, is_q ? gamma_q : gamma_k, eps, cos_t, sin_t, p, head_dim, lane);
}

// lane_rope_scatter_kernel with the head norm: one workgroup per lane, its four waves stride over the lane's heads; Q in place in
// the staging row, K into row pos[lane] of the lane's cache, V copied there.  Frozen lanes and positions outside the cache write nothing.
__global__ __launch_bounds__(256) void lane_qk_norm_rope_scatter_kernel(float* __restrict__ qkv, int64_t ld, int n_heads, int n_kv_heads,
                                                                        int head_dim, const float* __restrict__ gamma_q,
                                                                        const float* __restrict__ gamma_k, float eps,
                                                                        const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                        float* __restrict__ Kc, float* __restrict__ Vc, int64_t lane_stride,
                                                                        int capacity, const int* __restrict__ pos,
                                                                        const int* __restrict__ live)
{
    const int ln = blockIdx.x;
    if (!live[ln]) return;
    const int p = pos[ln];
    if (p < 0 || p >= capacity) return;
    const int qd = n_heads * head_dim, kv = n_kv_heads * head_dim;
    float* row = qkv + (int64_t)ln * ld;
    float* kdst = Kc + (int64_t)ln * lane_stride + (int64_t)p * kv;
    float* vdst = Vc + (int64_t)ln * lane_stride + (int64_t)p * kv;
    const int lane = threadIdx.x & 63;
    for (int h = threadIdx.x >> 6; h < n_heads + n_kv_heads; h += 4) {  // (uniform over the wave)
        if (h < n_heads) head_norm_rope(row + h * head_dim, row + h * head_dim, gamma_q, eps, cos_t, sin_t, p, head_dim, lane);
        else head_norm_rope(row + qd + (h - n_heads) * head_dim, kdst + (h - n_heads) * head_dim, gamma_k, eps, cos_t, sin_t, p, head_dim, lane);
    }
    for (int i = threadIdx.x; i < kv; i += 256) vdst[i] = row[qd + kv + i];
}

}  // namespace

hipError_t launch_qk_norm_rope(float* q, int64_t ldq, float* k, int64_t ldk, int rows, int n_heads, int n_kv_heads, int head_dim,
                               const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t, int pos,
                               const int* pos_ptr, int k_at_cache_row, hipStream_t stream)
{
    if (rows <= 0 || n_heads + n_kv_heads <= 0) return hipSuccess;
    if (n_heads < 0 || n_kv_heads < 0 || head_dim < 2 || head_dim > 128 || (head_dim & 1)) return hipErrorInvalidValue;
    const int64_t jobs = (int64_t)rows * (n_heads + n_kv_heads);
    if (jobs > (int64_t)1 << 30) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, stream, q, ldq, k, ldk, rows, n_heads, n_kv_heads,
                       head_dim, gamma_q, gamma_k, eps, cos_t, sin_t, pos, pos_ptr, k_at_cache_row);
    return hipGetLastError();
}

hipError_t launch_lane_qk_norm_rope_scatter(float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                            const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                            float* k_cache, float* v_cache, int64_t lane_stride, int capacity, LaneStateRef state,
                                            hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (lanes > state.width || head_dim < 2 || head_dim > 128 || (head_dim & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lane_qk_norm_rope_scatter_kernel, dim3((unsigned)lanes), dim3(256), 0, stream, qkv, ld, n_heads, n_kv_heads, head_dim,
                       gamma_q, gamma_k, eps, cos_t, sin_t, k_cache, v_cache, lane_stride, capacity, state.pos, state.live);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Prompt-lookup decoding (llm.cpp: LlmModel::generate_lookup): the draft of the next verify step, and its pick.
namespace {

constexpr int LOOKUP_THREADS = 1024;

// The draft rule on the history T[0, n) (n = st->n; T[n - 1] is the token that is not in the cache yet): over every e in
// [1, n) with a match of length m in [ngram_min, ngram_max] that ends just before e against the suffix of T, the largest
// (m, min(D, n - e), e) -- longest match, then longest continuation, then latest -- packed into one u64 and reduced with
// max, which is order-free: the result does not depend on how the threads share the positions.  One workgroup; it loops
// over a long history (131 072 tokens: 128 positions per thread, at most ngram_max + 1 loads each).
// ids[0] = T[n - 1], ids[1..c] = T[e .. e + c), rows past the draft repeat the last valid id; st->m = c.
__global__ __launch_bounds__(LOOKUP_THREADS) void lookup_draft_kernel(const int32_t* __restrict__ T, LlmLookupState* __restrict__ st,
                                                                      int ngram_max, int ngram_min, int D, int rows,
                                                                      uint32_t* __restrict__ ids)
{
    __shared__ unsigned long long red[LOOKUP_THREADS / kWave];
    const int n = st->n, tid = threadIdx.x;
    unsigned long long key = 0ull;  // (every valid key has m >= 1: non-zero)
    for (int e = 1 + tid; e < n; e += LOOKUP_THREADS) {
        int m = 0;
        while (m < ngram_max && e - 1 - m >= 0 && T[e - 1 - m] == T[n - 1 - m]) ++m;
        if (m < ngram_min) continue;
        const int c = min(D, n - e);
        const unsigned long long k = ((unsigned long long)m << 40) | ((unsigned long long)c << 32) | (uint32_t)e;
        key = k > key ? k : key;
    }
    key = wave_max_key(key);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;
    __syncthreads();
    if (tid >= rows) return;
    key = red[0];
    for (int w = 1; w < LOOKUP_THREADS / kWave; ++w) key = red[w] > key ? red[w] : key;
    int c = (int)((key >> 32) & 0xFFull);
    c = c < rows - 1 ? c : rows - 1;
    const int e = (int)(uint32_t)(key & 0xFFFFFFFFull);
    int src = n - 1;                               // row 0, and the pad rows of an empty draft
    if (tid > 0 && c > 0) src = e + (tid <= c ? tid : c) - 1;
    ids[tid] = n > 0 ? (uint32_t)T[src] : 0u;
    if (tid == 0) st->m = c;
}

// The verify pick: p_i = argmax(row i); a = the longest prefix of the draft with ids[1 + i] == p_i; p_0..p_a are the model's
// own greedy tokens after the history, so they join it (and st->picks), the position advances by a + 1 (the rows of the
// rejected and pad positions lie beyond it and are overwritten by the next step), and (m, a) joins the step log.
__global__ void lookup_pick_kernel(unsigned long long* __restrict__ best, const uint32_t* __restrict__ ids, int rows,
                                   LlmLookupState* __restrict__ st, int32_t* __restrict__ history, int hist_cap, int* __restrict__ pos,
                                   int32_t* __restrict__ log, int log_cap)
{
    if (threadIdx.x != 0) return;
    int32_t p[LLM_MAX_ROWS];
    for (int i = 0; i < rows; ++i) {
        p[i] = (int32_t)(uint32_t)(best[i] & 0xFFFFFFFFull);
        best[i] = 0ull;
    }
    int m = st->m;
    m = m < rows - 1 ? m : rows - 1;
    int a = 0;
    while (a < m && ids[1 + a] == (uint32_t)p[a]) ++a;
    const int n = st->n;
    for (int i = 0; i <= a; ++i) {
        st->picks[i] = p[i];
        if (history && n + i < hist_cap) history[n + i] = p[i];
    }
    st->n = n + a + 1;
    st->a = a;
    *pos += a + 1;
    const int s = st->steps;
    if (log && s < log_cap) {
        log[2 * s] = m;
        log[2 * s + 1] = a;
    }
    st->steps = s + 1;
}

}  // namespace

hipError_t launch_lookup_draft(const int32_t* history, LlmLookupState* state, int ngram_max, int ngram_min, int draft_tokens, int rows,
                               uint32_t* ids, hipStream_t stream)
{
    if (rows < 1 || rows > LLM_MAX_ROWS || ngram_max < 1 || ngram_max > kLookupMaxNgram || ngram_min < 1 || ngram_min > ngram_max ||
        draft_tokens < 0 || draft_tokens > rows - 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookup_draft_kernel, dim3(1), dim3(LOOKUP_THREADS), 0, stream, history, state, ngram_max, ngram_min, draft_tokens, rows,
                       ids);
    return hipGetLastError();
}

hipError_t launch_lookup_pick(const float* logits, int64_t ld, int vocab, int rows, const uint32_t* ids, unsigned long long* best_scratch,
                              LlmLookupState* state, int32_t* history, int hist_cap, int* pos, int32_t* log, int log_cap, hipStream_t stream)
{
    if (rows < 1 || rows > LLM_MAX_ROWS) return hipErrorInvalidValue;
    int blocks = (vocab + 2047) / 2048;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(argmax_partial_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, stream, logits, ld, vocab, 0,
                       static_cast<const int*>(nullptr), best_scratch);
    hipLaunchKernelGGL(lookup_pick_kernel, dim3(1), dim3(64), 0, stream, best_scratch, ids, rows, state, history, hist_cap, pos, log, log_cap);
    return hipGetLastError();
}

// ---- scoring: log-softmax statistics of every row's vocabulary logits (LlmModel::score) -------------------------------------
//   final norm + head   crates/kjarni-models/src/models/llama/cpu_decoder.rs:196-219, gpt2/cpu_decoder.rs:371-394
//   log_softmax_1d      crates/kjarni-transformers/src/common/sampling.rs:200-205 (x - max - ln(sum exp(x - max)))

namespace {

constexpr int SC_BM = 64, SC_BN = 64, SC_BK = 32, SC_STRIDE = SC_BK + 4;

// What one slab of vocabulary tiles knows about one row.
struct ScorePartial {
    unsigned long long key;  // argmax_key of the slab's best logit (0: nothing seen)
    float mx;                // the slab's maximum
    float sm;                // sum of exp(x - mx) over the slab
    float tgt;               // the target's logit where the target lies in the slab, else 0
    float pad;
};

__device__ __forceinline__ float argmax_key_value(unsigned long long key)
{
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// (mx, sm) += (omx, osm): sums of exp(x - mx) brought to the common maximum.
__device__ __forceinline__ void score_combine(float& mx, float& sm, float omx, float osm)
{
    const float m = fmaxf(mx, omx);
    if (m == -INFINITY) return;  // both empty
    sm = sm * expf(mx - m) + osm * expf(omx - m);
    mx = m;
}

// Top-k lists: TOPK argmax_keys in descending order, every index static so that the list lives in registers; 0 marks an empty
// slot.  Keys of different columns differ, so "the TOPK largest keys" is one set whatever the order of the insertions.
constexpr int SC_TOPK = KJARNI_SCORE_TOPK_MAX;

template <int TOPK>
__device__ __forceinline__ void topk_insert(unsigned long long (&lst)[TOPK], unsigned long long kk)
{
    if (kk > lst[TOPK - 1]) {  // the one compare of the common path
#pragma unroll
        for (int j = TOPK - 1; j > 0; --j) lst[j] = kk > lst[j - 1] ? lst[j - 1] : (kk > lst[j] ? kk : lst[j]);
        lst[0] = kk > lst[0] ? kk : lst[0];
    }
}

// lst = the TOPK largest of lst and the list lane ^ off holds; every lane of a pair ends with the same list.
template <int TOPK>
__device__ __forceinline__ void topk_merge_lane(unsigned long long (&lst)[TOPK], int off)
{
    unsigned long long o[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) o[j] = __shfl_xor(lst[j], off, kWave);
#pragma unroll
    for (int j = 0; j < TOPK; ++j) topk_insert(lst, o[j]);
}

// Eight consecutive weights of a row as two f32x4 (bf16 widened).
__device__ __forceinline__ void score_load_w(const float* p, f32x4& a, f32x4& b)
{
    a = *reinterpret_cast<const f32x4*>(p);
    b = *reinterpret_cast<const f32x4*>(p + 4);
}
__device__ __forceinline__ void score_load_w(const uint16_t* p, f32x4& a, f32x4& b)
{
    const F8 w = load8(p, 0);
    a = f32x4{w.v[0], w.v[1], w.v[2], w.v[3]};
    b = f32x4{w.v[4], w.v[5], w.v[6], w.v[7]};
}

// The vocabulary head without its output: for 64 rows of X[M, K] (final-normed hidden states) and a slab of `slab_tiles`
// consecutive 64-wide tiles of W[N, K] (f32 or bf16, widened while staged), the slab's running maximum, sum of exponentials,
// best (value, index) and the target's logit per row -- the [M, N] logits are never stored.  The structure is
// prefill_gemm_kernel's (4 waves, one 32 x 32 MFMA tile each, BK = 32 operand tiles double-buffered in LDS with the next
// tile's global loads in flight during the MFMAs, v_mfma_f32_32x32x2_f32: an exact k-ordered f32 fma chain), computing the
// transposed tile W . X^T, so that lane == row: a lane's 16 accumulators are 16 vocabulary entries of its own row and the
// reduction stays inside the lane until the slab ends, where the two half-waves (shuffle) and the two waves that share
// rows (LDS) meet once.  Columns >= N contribute nothing (their loads are clamped), rows >= M are not stored.
// TOPK > 0: every lane also keeps the TOPK largest keys it has seen (topk_insert; lst[0] is `key`), the lists merge where
// the single key does -- the second wave's through the first stage of sW, which nobody reads after the last tile -- and the
// workgroup writes them behind the partials, [row tile][slab][slot][row].  mx / sm / tgt are computed exactly as without.
template <typename WT, int TOPK>
__global__ __launch_bounds__(256) void llm_score_head_kernel(const float* __restrict__ X, int64_t ldx, const WT* __restrict__ W,
                                                             const uint32_t* __restrict__ targets, int M, int N, int K, int m_tiles,
                                                             int slab_tiles, int n_tiles, int slabs, ScorePartial* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) float sW[2][SC_BN * SC_STRIDE];
    __shared__ __attribute__((aligned(16))) float sX[2][SC_BM * SC_STRIDE];
    __shared__ ScorePartial sRed[SC_BM];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wv = wid >> 1, wx = wid & 1, l31 = lane & 31, half = lane >> 5;
    // XCD-aware order (prefill_gemm_kernel): every XCD takes one contiguous run of workgroups, row tiles fastest, so the
    // workgroups that stream the same slab of W sit behind the same L2
    const int64_t nwg = gridDim.x;
    const int64_t xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int64_t q8 = nwg / 8, r8 = nwg % 8;
    const int64_t bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    const int mt = (int)(bid % m_tiles), slab = (int)(bid / m_tiles);
    const int m0 = mt * SC_BM;
    const int t_begin = slab * slab_tiles, t_end = min(t_begin + slab_tiles, n_tiles);

    // X: 64 x 32 floats = 512 float4, two per thread.  W: 64 rows x 32 weights, eight consecutive ones per thread.
    const int a_row = tid >> 3, a_c4 = tid & 7;
    const float* x_ptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) x_ptr[i] = X + (int64_t)min(m0 + a_row + 32 * i, M - 1) * ldx + a_c4 * 4;
    const int w_row = tid >> 2, w_c = (tid & 3) * 8;
    const WT* w_ptr = W;
    f32x4 gx[2], gw[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) gx[i] = *reinterpret_cast<const f32x4*>(x_ptr[i] + k0);
        score_load_w(w_ptr + k0, gw[0], gw[1]);
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&sX[stage][(a_row + 32 * i) * SC_STRIDE + a_c4 * 4]) = gx[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&sW[stage][w_row * SC_STRIDE + w_c + 4 * i]) = gw[i];
    };

    const int row = m0 + wx * 32 + l31;
    const uint32_t target = (targets && row < M) ? targets[row] : 0xFFFFFFFFu;
    float mx = -INFINITY, sm = 0.0f, tgt = 0.0f;
    unsigned long long key = 0ull;
    [[maybe_unused]] unsigned long long lst[TOPK > 0 ? TOPK : 1];
    if constexpr (TOPK > 0) {
#pragma unroll
        for (int j = 0; j < TOPK; ++j) lst[j] = 0ull;
    }
    const int nk = K / SC_BK;
    const int fw = (wv * 32 + l31) * SC_STRIDE + half * 4, fx = (wx * 32 + l31) * SC_STRIDE + half * 4;
    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * SC_BN;
        w_ptr = W + (int64_t)min(n0 + w_row, N - 1) * K + w_c;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        load(0);
        store(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) load((kt + 1) * SC_BK);
#pragma unroll
            for (int kk = 0; kk < SC_BK / 8; ++kk) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&sW[cur][fw + kk * 8]);
                const f32x4 b = *reinterpret_cast<const f32x4*>(&sX[cur][fx + kk * 8]);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
            }
            if (kt + 1 < nk) store(cur ^ 1);
            __syncthreads();
        }
        // acc[r] = logit of (row, n0 + wv * 32 + acc_row(r, half)): fold the 16 into the lane's running state
        const int c0 = n0 + wv * 32;
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int col = c0 + acc_row(r, half);
            if (col < N) {
                tmax = fmaxf(tmax, acc[r]);
                const unsigned long long kk = argmax_key(acc[r], col);
                if constexpr (TOPK > 0) topk_insert(lst, kk);
                else key = kk > key ? kk : key;
                if ((uint32_t)col == target) tgt = acc[r];
            }
        }
        if (tmax > -INFINITY) {
            const float nm = fmaxf(mx, tmax);
            float ts = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (c0 + acc_row(r, half) < N) ts += expf(acc[r] - nm);
            sm = sm * expf(mx - nm) + ts;
            mx = nm;
        }
    }
    // the two half-waves of a row, then the two waves
    {
        const float omx = __shfl_xor(mx, 32, kWave), osm = __shfl_xor(sm, 32, kWave), otg = __shfl_xor(tgt, 32, kWave);
        score_combine(mx, sm, omx, osm);
        tgt += otg;  // at most one of them is not 0
        if constexpr (TOPK > 0) {
            topk_merge_lane(lst, 32);
            key = lst[0];
        } else {
            const unsigned long long ok = __shfl_xor(key, 32, kWave);
            key = ok > key ? ok : key;
        }
    }
    [[maybe_unused]] unsigned long long* sKeys = reinterpret_cast<unsigned long long*>(&sW[0][0]);  // [TOPK][SC_BM], free after the last tile
    if (wv == 1 && half == 0) {
        sRed[wx * 32 + l31] = ScorePartial{key, mx, sm, tgt, 0.0f};
        if constexpr (TOPK > 0) {
#pragma unroll
            for (int j = 0; j < TOPK; ++j) sKeys[j * SC_BM + wx * 32 + l31] = lst[j];
        }
    }
    __syncthreads();
    if (wv == 0 && half == 0 && row < M) {
        const ScorePartial o = sRed[wx * 32 + l31];
        score_combine(mx, sm, o.mx, o.sm);
        tgt += o.tgt;
        if constexpr (TOPK > 0) {
#pragma unroll
            for (int j = 0; j < TOPK; ++j) topk_insert(lst, sKeys[j * SC_BM + wx * 32 + l31]);
            key = lst[0];
            unsigned long long* PK = reinterpret_cast<unsigned long long*>(P + (int64_t)m_tiles * slabs * SC_BM);
#pragma unroll
            for (int j = 0; j < TOPK; ++j) PK[(((int64_t)mt * slabs + slab) * TOPK + j) * SC_BM + wx * 32 + l31] = lst[j];
        } else {
            key = o.key > key ? o.key : key;
        }
        P[((int64_t)mt * slabs + slab) * SC_BM + wx * 32 + l31] = ScorePartial{key, mx, sm, tgt, 0.0f};
    }
}

// One thread per row: the slab partials in slab order.  M = max mx, S = sum sm exp(mx - M), lse = M + log S.
__global__ __launch_bounds__(256) void llm_score_merge_kernel(const ScorePartial* __restrict__ P, const uint32_t* __restrict__ targets, int M,
                                                              int vocab, int slabs, int slab_tiles, float* __restrict__ logprob,
                                                              uint32_t* __restrict__ top, float* __restrict__ top_logprob,
                                                              float* __restrict__ lse_out)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= M) return;
    const ScorePartial* p = P + (int64_t)(row / SC_BM) * slabs * SC_BM + row % SC_BM;
    float mx = -INFINITY;
    unsigned long long key = 0ull;
    for (int s = 0; s < slabs; ++s) {
        const ScorePartial q = p[(int64_t)s * SC_BM];
        mx = fmaxf(mx, q.mx);
        key = q.key > key ? q.key : key;
    }
    float sum = 0.0f;
    for (int s = 0; s < slabs; ++s) {
        const ScorePartial q = p[(int64_t)s * SC_BM];
        sum += q.sm * expf(q.mx - mx);
    }
    const float lse = mx + logf(sum);
    if (lse_out) lse_out[row] = lse;
    if (top) top[row] = (uint32_t)(key & 0xFFFFFFFFull);
    if (top_logprob) top_logprob[row] = argmax_key_value(key) - lse;
    if (logprob && targets) {
        const uint32_t t = targets[row];
        logprob[row] = t < (uint32_t)vocab ? p[(int64_t)((int)(t / SC_BN) / slab_tiles) * SC_BM].tgt - lse : -INFINITY;
    }
}

// The slabs' top-k lists of one row into the row's: a wave per row (four rows per workgroup).  Lane l walks the slabs l, l + 64,
// ... in order, then the 64 lists meet in six butterfly steps (topk_merge_lane), after which every lane holds the row's list.
// Lane j < top_k writes slot j: the key's index, and its value less the lse llm_score_merge_kernel left for the row.
template <int TOPK>
__global__ __launch_bounds__(256) void llm_score_topk_merge_kernel(const unsigned long long* __restrict__ PK, const float* __restrict__ lse,
                                                                   int M, int slabs, int top_k, uint32_t* __restrict__ topk_ids,
                                                                   float* __restrict__ topk_logprob)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;  // (the whole wave)
    const unsigned long long* p = PK + (int64_t)(row / SC_BM) * slabs * TOPK * SC_BM + row % SC_BM;
    unsigned long long lst[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) lst[j] = 0ull;
    for (int s = lane; s < slabs; s += 64) {
#pragma unroll
        for (int j = 0; j < TOPK; ++j) topk_insert(lst, p[((int64_t)s * TOPK + j) * SC_BM]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) topk_merge_lane(lst, off);
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < TOPK; ++j) mine = lane == j ? lst[j] : mine;
    if (lane < top_k) {
        if (topk_ids) topk_ids[(int64_t)row * top_k + lane] = (uint32_t)(mine & 0xFFFFFFFFull);
        if (topk_logprob) topk_logprob[(int64_t)row * top_k + lane] = argmax_key_value(mine) - lse[row];
    }
}

// The same statistics from materialised logits [rows, ld]: one workgroup per row, the maximum (with its index, last one
// winning) first, then the sum of exp(x - max); both reduced lane -> wave -> workgroup in a fixed order.
// TOPK > 0: the first pass keeps a list per thread over its strided elements instead of the one key, merged lane -> wave
// (butterfly) -> workgroup (the four waves' lists through LDS, in wave order); lst[0] is the key, the rest is unchanged.
template <int TOPK>
__global__ __launch_bounds__(256) void llm_score_rows_kernel(const float* __restrict__ logits, int64_t ld, int vocab,
                                                             const uint32_t* __restrict__ targets, float* __restrict__ logprob,
                                                             uint32_t* __restrict__ top, float* __restrict__ top_logprob,
                                                             float* __restrict__ lse_out, int top_k, uint32_t* __restrict__ topk_ids,
                                                             float* __restrict__ topk_logprob)
{
    __shared__ unsigned long long red_key[TOPK > 0 ? 4 * TOPK : 4];
    __shared__ float red_sum[4];
    const float* row = logits + (int64_t)blockIdx.x * ld;
    unsigned long long key = 0ull;
    [[maybe_unused]] unsigned long long lst[TOPK > 0 ? TOPK : 1];
    if constexpr (TOPK > 0) {
#pragma unroll
        for (int j = 0; j < TOPK; ++j) lst[j] = 0ull;
        for (int i = threadIdx.x; i < vocab; i += 256) topk_insert(lst, argmax_key(row[i], i));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) topk_merge_lane(lst, off);
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int j = 0; j < TOPK; ++j) red_key[(threadIdx.x >> 6) * TOPK + j] = lst[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TOPK; ++j) lst[j] = red_key[j];
        for (int w = 1; w < 4; ++w) {
#pragma unroll
            for (int j = 0; j < TOPK; ++j) topk_insert(lst, red_key[w * TOPK + j]);
        }
        key = lst[0];
    } else {
        for (int i = threadIdx.x; i < vocab; i += 256) {
            const unsigned long long kk = argmax_key(row[i], i);
            key = kk > key ? kk : key;
        }
        key = wave_max_key(key);
        if ((threadIdx.x & 63) == 0) red_key[threadIdx.x >> 6] = key;
        __syncthreads();
        key = red_key[0];
        for (int w = 1; w < 4; ++w) key = red_key[w] > key ? red_key[w] : key;
    }
    const float mx = argmax_key_value(key);
    float sum = 0.0f;
    for (int i = threadIdx.x; i < vocab; i += 256) sum += expf(row[i] - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
    if ((threadIdx.x & 63) == 0) red_sum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float lse = mx + logf((red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3]));
    const int r = blockIdx.x;
    if (lse_out) lse_out[r] = lse;
    if (top) top[r] = (uint32_t)(key & 0xFFFFFFFFull);
    if (top_logprob) top_logprob[r] = mx - lse;
    if (logprob && targets) logprob[r] = targets[r] < (uint32_t)vocab ? row[targets[r]] - lse : -INFINITY;
    if constexpr (TOPK > 0) {
#pragma unroll
        for (int j = 0; j < TOPK; ++j) {
            if (topk_ids && j < top_k) topk_ids[(int64_t)r * top_k + j] = (uint32_t)(lst[j] & 0xFFFFFFFFull);
            if (topk_logprob && j < top_k) topk_logprob[(int64_t)r * top_k + j] = argmax_key_value(lst[j]) - lse;
        }
    }
}

}  // namespace

bool llm_score_head_takes(const float* X, int64_t ldx, const void* W, int bf16, int k)
{
    return k > 0 && k % SC_BK == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0 &&
           (bf16 == 0 || bf16 == 1);
}

int score_head_slab_tiles(int m, int vocab, int slab_tiles)
{
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    if (slab_tiles > 0) return std::min(slab_tiles, n_tiles);
    // four workgroups per CU (their LDS allows that many): row tiles x slabs >= 1 024 where the vocabulary has the tiles
    const int slabs = std::max(1, std::min(n_tiles, (1024 + m_tiles - 1) / m_tiles));
    return (n_tiles + slabs - 1) / slabs;
}

size_t score_head_scratch_bytes(int m, int vocab, int slab_tiles)
{
    if (m <= 0 || vocab <= 0) return 0;
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    const int st = score_head_slab_tiles(m, vocab, slab_tiles);
    return (size_t)m_tiles * ((n_tiles + st - 1) / st) * SC_BM * sizeof(ScorePartial);
}

// scratch of the top-k launch: the partials, the slabs' lists (SC_TOPK keys each, whatever top_k), one lse per row
size_t score_head_topk_scratch_bytes(int m, int vocab, int slab_tiles, int top_k)
{
    if (top_k < 1 || top_k > SC_TOPK) return 0;
    const size_t partials = score_head_scratch_bytes(m, vocab, slab_tiles);
    return partials + partials / sizeof(ScorePartial) * SC_TOPK * sizeof(unsigned long long) + (size_t)std::max(m, 0) * sizeof(float);
}

hipError_t launch_score_head_topk(const float* X, int64_t ldx, int m, const void* W, int bf16, int vocab, int k, const uint32_t* targets,
                                  int slab_tiles, int top_k, void* scratch, float* logprob, uint32_t* topk_ids, float* topk_logprob, float* lse,
                                  hipStream_t stream)
{
    if (m <= 0) return hipSuccess;
    if (vocab <= 0 || top_k < 1 || top_k > SC_TOPK || top_k > vocab || !scratch || !llm_score_head_takes(X, ldx, W, bf16, k))
        return hipErrorInvalidValue;
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    const int st = score_head_slab_tiles(m, vocab, slab_tiles);
    const int slabs = (n_tiles + st - 1) / st;
    ScorePartial* P = static_cast<ScorePartial*>(scratch);
    const unsigned long long* PK = reinterpret_cast<const unsigned long long*>(P + (int64_t)m_tiles * slabs * SC_BM);  // where the kernel writes
    float* row_lse = lse ? lse : const_cast<float*>(reinterpret_cast<const float*>(PK + (int64_t)m_tiles * slabs * SC_TOPK * SC_BM));
    const dim3 grid((unsigned)(m_tiles * slabs));
    if (bf16)
        hipLaunchKernelGGL((llm_score_head_kernel<uint16_t, SC_TOPK>), grid, dim3(256), 0, stream, X, ldx, static_cast<const uint16_t*>(W), targets,
                           m, vocab, k, m_tiles, st, n_tiles, slabs, P);
    else
        hipLaunchKernelGGL((llm_score_head_kernel<float, SC_TOPK>), grid, dim3(256), 0, stream, X, ldx, static_cast<const float*>(W), targets, m,
                           vocab, k, m_tiles, st, n_tiles, slabs, P);
    // logprob and lse by score()'s own merge, in its order; then the lists
    hipLaunchKernelGGL(llm_score_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, P, targets, m, vocab, slabs, st, logprob,
                       static_cast<uint32_t*>(nullptr), static_cast<float*>(nullptr), row_lse);
    hipLaunchKernelGGL(llm_score_topk_merge_kernel<SC_TOPK>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, stream, PK, row_lse, m, slabs, top_k,
                       topk_ids, topk_logprob);
    return hipGetLastError();
}

hipError_t launch_score_head(const float* X, int64_t ldx, int m, const void* W, int bf16, int vocab, int k, const uint32_t* targets,
                             int slab_tiles, void* scratch, float* logprob, uint32_t* top, float* top_logprob, float* lse, hipStream_t stream)
{
    if (m <= 0) return hipSuccess;
    if (vocab <= 0 || !scratch || !llm_score_head_takes(X, ldx, W, bf16, k)) return hipErrorInvalidValue;
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    const int st = score_head_slab_tiles(m, vocab, slab_tiles);
    const int slabs = (n_tiles + st - 1) / st;
    ScorePartial* P = static_cast<ScorePartial*>(scratch);
    const dim3 grid((unsigned)(m_tiles * slabs));
    if (bf16)
        hipLaunchKernelGGL((llm_score_head_kernel<uint16_t, 0>), grid, dim3(256), 0, stream, X, ldx, static_cast<const uint16_t*>(W), targets, m,
                           vocab, k, m_tiles, st, n_tiles, slabs, P);
    else
        hipLaunchKernelGGL((llm_score_head_kernel<float, 0>), grid, dim3(256), 0, stream, X, ldx, static_cast<const float*>(W), targets, m, vocab,
                           k, m_tiles, st, n_tiles, slabs, P);
    hipLaunchKernelGGL(llm_score_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, P, targets, m, vocab, slabs, st, logprob, top,
                       top_logprob, lse);
    return hipGetLastError();
}

hipError_t launch_score_rows(const float* logits, int64_t ld, int rows, int vocab, const uint32_t* targets, float* logprob, uint32_t* top,
                             float* top_logprob, float* lse, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (rows > LLM_MAX_ROWS || vocab <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_score_rows_kernel<0>, dim3((unsigned)rows), dim3(256), 0, stream, logits, ld, vocab, targets, logprob, top, top_logprob,
                       lse, 0, static_cast<uint32_t*>(nullptr), static_cast<float*>(nullptr));
    return hipGetLastError();
}

hipError_t launch_score_rows_topk(const float* logits, int64_t ld, int rows, int vocab, const uint32_t* targets, int top_k, float* logprob,
                                  uint32_t* topk_ids, float* topk_logprob, float* lse, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (rows > LLM_MAX_ROWS || vocab <= 0 || top_k < 1 || top_k > SC_TOPK || top_k > vocab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_score_rows_kernel<SC_TOPK>, dim3((unsigned)rows), dim3(256), 0, stream, logits, ld, vocab, targets, logprob,
                       static_cast<uint32_t*>(nullptr), static_cast<float*>(nullptr), lse, top_k, topk_ids, topk_logprob);
    return hipGetLastError();
}

// ---- sampled prompt-lookup decoding (LlmModel::generate_lookup_sampled): the sampler's cut and the repetition penalty over the
// rows of a verify block are the kernels of sampled decoding above with rows in blockIdx.y; the commit of a step's picks.
namespace {

// The host's decision of a sampled verify step joins the device state: up[0] = how many picks, up[1..] = the picks.
__global__ void lookup_commit_kernel(const int32_t* __restrict__ up, LlmLookupState* __restrict__ st, int32_t* __restrict__ history,
                                     int hist_cap, int* __restrict__ pos)
{
    if (threadIdx.x != 0) return;
    int k = up[0];
    k = k < 0 ? 0 : (k > LLM_MAX_ROWS ? LLM_MAX_ROWS : k);
    const int n = st->n;
    for (int i = 0; i < k; ++i)
        if (n + i < hist_cap) history[n + i] = up[1 + i];
    st->n = n + k;
    *pos += k;
}

}  // namespace

size_t sample_scratch_rows_bytes(int rows) { return (size_t)(rows > 0 ? rows : 0) * sizeof(SampleScratch); }

hipError_t launch_sample_candidates_rows(const float* logits, int64_t ld, int rows, int vocab, int64_t top_k, float top_p, float min_p,
                                         void* scratch, SampleHeader* headers, SampleCandidate* candidates, int capacity, hipStream_t stream)
{
    if (rows < 1 || rows > LLM_MAX_ROWS || vocab < 1 || ld < (int64_t)vocab || capacity < 1) return hipErrorInvalidValue;
    return launch_sample_cut(logits, ld, rows, vocab, top_k, top_p, min_p, scratch, headers, candidates, capacity, true, stream);
}

hipError_t launch_repetition_penalty_rows(float* logits, int64_t ld, int rows, int vocab, const uint32_t* ids, const int* counts,
                                          const int32_t* distinct, const int* n_distinct, float penalty, hipStream_t stream)
{
    if (rows < 1 || rows > LLM_MAX_ROWS || vocab < 1 || ld < (int64_t)vocab) return hipErrorInvalidValue;
    if (penalty == 1.0f) return hipSuccess;
    hipLaunchKernelGGL(repetition_penalty_kernel, dim3(16, (unsigned)rows), dim3(256), 0, stream, logits, ld, vocab, ids, counts, distinct,
                       n_distinct, penalty);
    return hipGetLastError();
}

hipError_t launch_lookup_commit(const int32_t* upload, LlmLookupState* state, int32_t* history, int hist_cap, int* pos, hipStream_t stream)
{
    hipLaunchKernelGGL(lookup_commit_kernel, dim3(1), dim3(64), 0, stream, upload, state, history, hist_cap, pos);
    return hipGetLastError();
}

}  // namespace kjarni
