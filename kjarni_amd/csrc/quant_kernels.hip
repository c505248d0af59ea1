// GGUF quantized matrices resident in HBM (gfx950): decode GEMV, Q8_K activation quantization, dequantization for the
// prompt route, embedding gather.
//
// Device layout.  GGUF blocks (Q8_0 34 B, Q6_K 210 B) are not aligned for wide loads, so every matrix [n, k] is repacked at
// load into planes, each its own 256-byte aligned allocation, rows in HF order, blocks of a row contiguous:
//   Q8_0  q  int8 [n, k]                    the codes
//         s  f32  [n, k / 32]               d of each 32-block (the f16 widened; exact)
//   Q4_K  q  u8   [n, k / 256, 128]         the block's qs bytes as stored (byte l of chunk j holds elements 64j + l (low
//                                           nibble) and 64j + 32 + l (high nibble))
//         s  f32  [n, k / 256, 16]          d * sc_j (j = 0..7), then dmin * m_j: the products dequantize.rs forms, so
//                                           w = (d*sc_j) * q - (dmin*m_j) rounds as the reference
//   Q6_K  q  u8   [n, k / 256, 128]         ql as stored
//         q2 u8   [n, k / 256, 64]          qh as stored
//         s  f32  [n, k / 256]              d
//         s2 int8 [n, k / 256, 16]          the sub-block scales as stored
//
// Decode GEMV (qfused_kernel).  One wave per job of two output columns; each lane takes a 16-byte unit of each column's quants
// plane per step (Q8_0: 16 weights, Q4_K: 32, Q6_K: 16 ql bytes of each of the two ql runs + 16 qh bytes = 64 weights), units
// of a row spread over the 64 lanes and two steps unrolled, so a wave streams two rows of weights straight into VGPRs (no LDS)
// with their loads in flight together, and the activation rows (<= 8, a few KB) come through the caches, RMS-normalised on the
// fly where the stage has a norm.  A wave-wide reduction and the stage's epilogue (bias, RoPE + cache write, SwiGLU,
// residual) finish the pair.  One launch per stage: QKV (per-segment types), o-proj, gate/up, down, head.
#include "quant_kernels.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "gguf.h"

namespace kjarni {

namespace {

constexpr int kWaves = 4;  // waves (columns) per workgroup

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int R>
__device__ inline void accum16(float (&acc)[R], const float* X, int64_t ldx, int rows, int64_t col, const float (&w)[16])
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < rows) {
            const float4* xp = reinterpret_cast<const float4*>(X + r * ldx + col);
            float a = acc[r];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 x = xp[c];
                a = fmaf(w[4 * c + 0], x.x, a);
                a = fmaf(w[4 * c + 1], x.y, a);
                a = fmaf(w[4 * c + 2], x.z, a);
                a = fmaf(w[4 * c + 3], x.w, a);
            }
            acc[r] = a;
        }
    }
}

__device__ inline void bytes16(const uint8_t* p, uint8_t (&b)[16])
{
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(u[i >> 2] >> (8 * (i & 3)));
}

__device__ inline uint4 ld16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }

// byte i (0..15, a compile-time constant after unrolling) of a 16-byte word
__device__ inline uint32_t byte_of(const uint4& v, int i)
{
    const uint32_t w = (i >> 2) == 0 ? v.x : ((i >> 2) == 1 ? v.y : ((i >> 2) == 2 ? v.z : v.w));
    return (w >> (8 * (i & 3))) & 0xFFu;
}

// Activation rows as a GEMV reads them: X [rows, ldx], normalised on the fly when gamma is set (x * (1 / rms) * gamma, rms per
// row from the workgroup's prologue), and the Q8_K codes of the same rows for Q6_K linears.
struct QSrc {
    const float* X;
    int64_t ldx;
    int rows, k;
    const float* gamma;
    const float* inv;  // [rows] 1 / rms (LDS)
    const int8_t* Xq;
    const float* Xd;
};

// 16 consecutive activations of row r from column col
__device__ inline void xrow16(const QSrc& x, int r, int64_t col, float (&v)[16])
{
    const float4* xp = reinterpret_cast<const float4*>(x.X + r * x.ldx + col);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float4 t = xp[c];
        v[4 * c] = t.x; v[4 * c + 1] = t.y; v[4 * c + 2] = t.z; v[4 * c + 3] = t.w;
    }
    if (x.gamma) {
        const float4* gp = reinterpret_cast<const float4*>(x.gamma + col);
        const float iv = x.inv[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 g = gp[c];
            v[4 * c] = v[4 * c] * iv * g.x; v[4 * c + 1] = v[4 * c + 1] * iv * g.y;
            v[4 * c + 2] = v[4 * c + 2] * iv * g.z; v[4 * c + 3] = v[4 * c + 3] * iv * g.w;
        }
    }
}

// acc_c[r] += sum_i w_c[i] x[r, col + i] for C columns sharing the activations
template <int C, int R>
__device__ inline void accum16(float (&acc)[C][R], const QSrc& x, int64_t col, const float (&w)[C][16])
{
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r < x.rows) {
            float v[16];
            xrow16(x, r, col, v);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float a = acc[c][r];
#pragma unroll
                for (int i = 0; i < 16; ++i) a = fmaf(w[c][i], v[i], a);
                acc[c][r] = a;
            }
        }
    }
}

// C columns (rows n[c] of matrices W[c], all of type T) against the activation rows: per-lane partial sums in acc (the
// wave-wide reduction follows).  Q8K: Q6_K x Q8_K codes in integers per 256-block, d_w * d_a applied once per block.
template <uint32_t T, bool Q8K, int C, int R>
__device__ inline void qcols(const QMat* const (&W)[C], const int (&n)[C], const QSrc& x, float (&acc)[C][R])
{
    const int lane = threadIdx.x & 63, k = x.k;
    if constexpr (T == GGML_Q8_0) {
        const int units = k / 16;
#pragma unroll 2
        for (int u = lane; u < units; u += 64) {
            uint4 b[C];
            float d[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                b[c] = ld16(static_cast<const uint8_t*>(W[c]->q) + (int64_t)n[c] * k + u * 16);
                d[c] = static_cast<const float*>(W[c]->s)[(int64_t)n[c] * (k / 32) + (u >> 1)];
            }
            float w[C][16];
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) w[c][i] = (float)(int8_t)byte_of(b[c], i) * d[c];
            accum16<C, R>(acc, x, (int64_t)u * 16, w);
        }
    } else if constexpr (T == GGML_Q4_K) {
        const int nb = k / 256, units = k / 32;
#pragma unroll 2
        for (int u = lane; u < units; u += 64) {
            const int blk = u >> 3, o = (u & 7) * 16, j = o >> 5, l = o & 31;
            uint4 b[C];
            float sc[C][4];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                b[c] = ld16(static_cast<const uint8_t*>(W[c]->q) + ((int64_t)n[c] * nb * 128) + (int64_t)u * 16);
                const float* sb = static_cast<const float*>(W[c]->s) + ((int64_t)n[c] * nb + blk) * 16;
                sc[c][0] = sb[2 * j]; sc[c][1] = sb[2 * j + 1]; sc[c][2] = sb[8 + 2 * j]; sc[c][3] = sb[8 + 2 * j + 1];
            }
            const int64_t col = (int64_t)blk * 256 + j * 64 + l;
            float w[C][16];
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) w[c][i] = __fsub_rn(__fmul_rn(sc[c][0], (float)(byte_of(b[c], i) & 0xF)), sc[c][2]);
            accum16<C, R>(acc, x, col, w);
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int i = 0; i < 16; ++i) w[c][i] = __fsub_rn(__fmul_rn(sc[c][1], (float)(byte_of(b[c], i) >> 4)), sc[c][3]);
            accum16<C, R>(acc, x, col + 32, w);
        }
    } else {  // Q6_K: 64 weights per lane and step; units a multiple of 4, so a block's 4 lanes are all in or all out
        const int nb = k / 256, units = k / 64;
        for (int base = 0; base < units; base += 64) {
            const int u = base + lane;
            const bool valid = u < units;
            const int blk = u >> 2, half = (u >> 1) & 1, k0 = (u & 1) * 16;
            uint4 A[C], B[C], H[C];
            int sc[C][4];
            float d[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = 0.0f;
#pragma unroll
                for (int g = 0; g < 4; ++g) sc[c][g] = 0;
                if (valid) {
                    const uint8_t* ql = static_cast<const uint8_t*>(W[c]->q) + ((int64_t)n[c] * nb + blk) * 128 + half * 64 + k0;
                    A[c] = ld16(ql);
                    B[c] = ld16(ql + 32);
                    H[c] = ld16(static_cast<const uint8_t*>(W[c]->q2) + ((int64_t)n[c] * nb + blk) * 64 + half * 32 + k0);
                    const int8_t* sb = static_cast<const int8_t*>(W[c]->s2) + ((int64_t)n[c] * nb + blk) * 16 + half * 8 + (k0 >> 4);
#pragma unroll
                    for (int g = 0; g < 4; ++g) sc[c][g] = sb[2 * g];
                    d[c] = static_cast<const float*>(W[c]->s)[(int64_t)n[c] * nb + blk];
                }
            }
            const int64_t col = (int64_t)blk * 256 + half * 128 + k0;
            if constexpr (Q8K) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    int sumi[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) sumi[c] = 0;
                    if (valid && r < x.rows) {
                        const int8_t* xq = x.Xq + (int64_t)r * k + col;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const uint4 xb = ld16(reinterpret_cast<const uint8_t*>(xq + 32 * g));
#pragma unroll
                            for (int c = 0; c < C; ++c) {
                                int part = 0;
#pragma unroll
                                for (int i = 0; i < 16; ++i) {
                                    const uint32_t lo = byte_of((g & 1) ? B[c] : A[c], i);
                                    const int nib = (int)((g < 2) ? (lo & 0xF) : (lo >> 4));
                                    const int qw = nib | (((byte_of(H[c], i) >> (2 * g)) & 3) << 4);
                                    part += (qw - 32) * (int)(int8_t)byte_of(xb, i);
                                }
                                sumi[c] += sc[c][g] * part;
                            }
                        }
                    }
                    // the block's integer sum over its 4 lanes, then d_w * d_a once per block (scalar.rs:179-240)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        int v = sumi[c];
                        v += __shfl_xor(v, 1, 64);
                        v += __shfl_xor(v, 2, 64);
                        if (valid && (u & 3) == 0 && r < x.rows) acc[c][r] += (d[c] * x.Xd[(int64_t)r * (k / 256) + blk]) * (float)v;
                    }
                }
            } else if (valid) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float w[C][16];
#pragma unroll
                    for (int c = 0; c < C; ++c)
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const uint32_t lo = byte_of((g & 1) ? B[c] : A[c], i);
                            const int nib = (int)((g < 2) ? (lo & 0xF) : (lo >> 4));
                            const int qw = (nib | (((byte_of(H[c], i) >> (2 * g)) & 3) << 4)) - 32;
                            w[c][i] = __fmul_rn(__fmul_rn(d[c], (float)qw), (float)sc[c][g]);
                        }
                    accum16<C, R>(acc, x, col + 32 * g, w);
                }
            }
        }
    }
}

// Two columns of the same type (or one, when W[1] is null); dispatch on the type (wave-uniform).
template <int R>
__device__ inline void qpair(const QMat* Wa, int na, const QMat* Wb, int nb, const QSrc& x, float (&out)[2][R])
{
    const bool pair = Wb && Wb->type == Wa->type;
    const bool q8k = x.Xq != nullptr;
#pragma unroll
    for (int r = 0; r < R; ++r) out[0][r] = out[1][r] = 0.0f;
    if (pair) {
        const QMat* const W[2] = {Wa, Wb};
        const int n[2] = {na, nb};
        switch (Wa->type) {
        case GGML_Q8_0: qcols<GGML_Q8_0, false, 2, R>(W, n, x, out); break;
        case GGML_Q4_K: qcols<GGML_Q4_K, false, 2, R>(W, n, x, out); break;
        default:
            if (q8k) qcols<GGML_Q6_K, true, 2, R>(W, n, x, out);
            else qcols<GGML_Q6_K, false, 2, R>(W, n, x, out);
        }
        return;
    }
    const QMat* Ws[2] = {Wa, Wb};
    const int ns[2] = {na, nb};
#pragma unroll
    for (int c = 0; c < 2; ++c) {  // one column at a time (a lone column, or gate / up of different types)
        if (!Ws[c]) continue;
        const QMat* const W[1] = {Ws[c]};
        const int n[1] = {ns[c]};
        float acc[1][R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[0][r] = 0.0f;
        switch (Ws[c]->type) {
        case GGML_Q8_0: qcols<GGML_Q8_0, false, 1, R>(W, n, x, acc); break;
        case GGML_Q4_K: qcols<GGML_Q4_K, false, 1, R>(W, n, x, acc); break;
        default:
            if (q8k) qcols<GGML_Q6_K, true, 1, R>(W, n, x, acc);
            else qcols<GGML_Q6_K, false, 1, R>(W, n, x, acc);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) out[c][r] = acc[0][r];
    }
}

// One wave per job of two columns (see QFusedArgs); 4 waves per workgroup.  With gamma the workgroup first computes the
// rows' 1 / rms (one wave per row, as rmsnorm_kernel).
template <int R>
__global__ __launch_bounds__(64 * kWaves) void qfused_kernel(QFusedArgs a)
{
    __shared__ float inv[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (a.gamma) {
        for (int r = wave; r < a.rows; r += kWaves) {
            const float* row = a.X + r * a.ldx;
            float s = 0.0f;
            for (int i = lane; i < a.k; i += 64) s = fmaf(row[i], row[i], s);
            s = wave_sum(s);
            if (lane == 0) inv[r] = 1.0f / sqrtf(s / (float)a.k + a.eps);
        }
        __syncthreads();
    }
    const QSrc x{a.X, a.ldx, a.rows, a.k, a.gamma, inv, a.Xq, a.Xd};
    const int job = blockIdx.x * kWaves + wave;
    if (job >= a.jobs) return;  // (a whole wave; no barrier follows)
    const int off = a.row_off_ptr ? *a.row_off_ptr : a.row_off;
    float v[2][R];
    if (a.mode == QF_SWIGLU) {  // gate column j and up column j: silu(gate) * up
        const QMat g = a.W[0], u = a.W[1];
        qpair<R>(&g, job, &u, job, x, v);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float g = wave_sum(v[0][r]), u = wave_sum(v[1][r]);
            if (lane == 0 && r < a.rows) a.Y[0][(int64_t)r * a.ldy[0] + job] = (g / (1.0f + expf(-g))) * u;
        }
        return;
    }
    // segment s of the concatenated output; QKV: Q and K jobs are (i, i + d/2) of one head, rotated together (RoPE)
    int s = 0, j = job;
    if (j >= a.seg_jobs[0]) {
        j -= a.seg_jobs[0];
        s = 1;
        if (j >= a.seg_jobs[1]) {
            j -= a.seg_jobs[1];
            s = 2;
        }
    }
    // (selected by value: a runtime index into the argument arrays would put them in scratch)
    const QMat Ws = s == 0 ? a.W[0] : (s == 1 ? a.W[1] : a.W[2]);
    const QMat* W = &Ws;
    const bool rope = a.mode == QF_QKV && s < 2;
    int c0, c1;
    if (rope) {
        const int half = a.head_dim / 2;
        c0 = (j / half) * a.head_dim + j % half;
        c1 = c0 + half;
    } else {
        c0 = 2 * j;
        c1 = 2 * j + 1;
    }
    const bool two = c1 < W->n;
    qpair<R>(W, c0, two ? W : nullptr, c1, x, v);
    const float* bias = a.bias ? a.bias + (s == 0 ? a.bias_off[0] : (s == 1 ? a.bias_off[1] : a.bias_off[2])) : nullptr;
    float* Y = s == 0 ? a.Y[0] : (s == 1 ? a.Y[1] : a.Y[2]);
    const int64_t ldy = s == 0 ? a.ldy[0] : (s == 1 ? a.ldy[1] : a.ldy[2]);
    const int base = (a.mode == QF_QKV && s > 0) ? off : 0;  // K / V rows land at the cache position
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float y0 = wave_sum(v[0][r]), y1 = wave_sum(v[1][r]);
        if (lane == 0 && r < a.rows) {
            if (bias) {
                y0 += bias[c0];
                if (two) y1 += bias[c1];
            }
            if (rope) {
                const int p = off + r, half = a.head_dim / 2, i = c0 % a.head_dim;
                const float cs = a.cos_t[(int64_t)p * half + i], sn = a.sin_t[(int64_t)p * half + i];
                const float x0 = y0, x1 = y1;
                y0 = x0 * cs - x1 * sn;
                y1 = x0 * sn + x1 * cs;
            }
            float* yr = Y + ((int64_t)base + r) * ldy;
            if (a.R) {
                y0 += a.R[(int64_t)r * a.ldr + c0];
                if (two) y1 += a.R[(int64_t)r * a.ldr + c1];
            }
            yr[c0] = y0;
            if (two) yr[c1] = y1;
        }
    }
}

// One wave per 256-block of one row (kernels/quantize.rs:57-126): d = amax / 127, q = round(x * (1 / d)), half away from zero.
__global__ __launch_bounds__(256) void q8k_quantize_kernel(const float* X, int64_t ldx, int rows, int k, int8_t* codes, float* scales,
                                                           float* deq)
{
    const int nb = k / 256;
    const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= rows * nb) return;
    const int r = blk / nb, b = blk % nb;
    const float4 x = *reinterpret_cast<const float4*>(X + r * ldx + b * 256 + lane * 4);
    float m = fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w)));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float d = 0.0f, inv = 0.0f;
    if (m != 0.0f) {
        d = __fdiv_rn(m, 127.0f);
        inv = __fdiv_rn(1.0f, d);
    }
    const float xv[4] = {x.x, x.y, x.z, x.w};
    int8_t q[4];
    float dq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float s = roundf(__fmul_rn(xv[i], inv));
        const int c = s >= 127.0f ? 127 : (s <= -128.0f ? -128 : (int)s);
        q[i] = (int8_t)c;
        dq[i] = __fmul_rn((float)c, d);
    }
    const int64_t o = (int64_t)r * k + b * 256 + lane * 4;
    uint32_t packed = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) packed |= (uint32_t)(uint8_t)q[i] << (8 * i);
    if (codes) *reinterpret_cast<uint32_t*>(codes + o) = packed;
    if (scales && lane == 0) scales[(int64_t)r * nb + b] = d;
    if (deq) *reinterpret_cast<float4*>(deq + o) = make_float4(dq[0], dq[1], dq[2], dq[3]);
}

// One workgroup per row: 1 / rms over the row (gamma set), then one wave per 256-block: normalised values (x / rms) * gamma,
// their Q8_K codes (as q8k_quantize_kernel).
__global__ __launch_bounds__(256) void qprep_kernel(const float* X, int64_t ldx, int k, const float* gamma, float eps, float* xn,
                                                    int8_t* codes, float* scales)
{
    __shared__ float red[4];
    const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = X + r * ldx;
    float rms = 1.0f;
    if (gamma) {
        float s = 0.0f;
        for (int i = threadIdx.x; i < k; i += 256) s = fmaf(row[i], row[i], s);
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        rms = sqrtf((red[0] + red[1] + red[2] + red[3]) / (float)k + eps);
    }
    const int nb = k / 256;
    for (int b = wave; b < nb; b += 4) {
        const int c = b * 256 + lane * 4;
        const float4 x4 = *reinterpret_cast<const float4*>(row + c);
        float xv[4] = {x4.x, x4.y, x4.z, x4.w};
        if (gamma) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            xv[0] = (xv[0] / rms) * g.x; xv[1] = (xv[1] / rms) * g.y; xv[2] = (xv[2] / rms) * g.z; xv[3] = (xv[3] / rms) * g.w;
        }
        if (xn) *reinterpret_cast<float4*>(xn + (int64_t)r * k + c) = make_float4(xv[0], xv[1], xv[2], xv[3]);
        if (!codes) continue;
        float m = fmaxf(fmaxf(fabsf(xv[0]), fabsf(xv[1])), fmaxf(fabsf(xv[2]), fabsf(xv[3])));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float d = 0.0f, iv = 0.0f;
        if (m != 0.0f) {
            d = __fdiv_rn(m, 127.0f);
            iv = __fdiv_rn(1.0f, d);
        }
        uint32_t packed = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float q = roundf(__fmul_rn(xv[i], iv));
            const int cq = q >= 127.0f ? 127 : (q <= -128.0f ? -128 : (int)q);
            packed |= (uint32_t)(uint8_t)(int8_t)cq << (8 * i);
        }
        *reinterpret_cast<uint32_t*>(codes + (int64_t)r * k + c) = packed;
        if (lane == 0) scales[(int64_t)r * nb + b] = d;
    }
}

// element (row, col) of a quantized matrix, dequantized with the reference's arithmetic
__device__ inline float q_element(const QMat& W, int64_t row, int col)
{
    const int k = W.k;
    if (W.type == GGML_Q8_0) {
        const int64_t i = row * k + col;
        return (float)static_cast<const int8_t*>(W.q)[i] * static_cast<const float*>(W.s)[i / 32];
    }
    const int nb = k / 256;
    const int64_t blk = row * nb + col / 256;
    const int e = col % 256;
    if (W.type == GGML_Q4_K) {
        const int j = e / 64, within = e % 64, hi = within >= 32, l = within % 32;
        const uint8_t byte = static_cast<const uint8_t*>(W.q)[blk * 128 + j * 32 + l];
        const int nib = hi ? (byte >> 4) : (byte & 0xF);
        const float* s = static_cast<const float*>(W.s) + blk * 16;
        return __fsub_rn(__fmul_rn(s[2 * j + hi], (float)nib), s[8 + 2 * j + hi]);
    }
    // Q6_K
    const int half = e / 128, e2 = e % 128, g = e2 / 32, kk = e2 % 32;
    const uint8_t lo = static_cast<const uint8_t*>(W.q)[blk * 128 + half * 64 + (g & 1) * 32 + kk];
    const uint8_t hb = static_cast<const uint8_t*>(W.q2)[blk * 64 + half * 32 + kk];
    const int nib = g < 2 ? (lo & 0xF) : (lo >> 4);
    const int qw = (nib | (((hb >> (2 * g)) & 3) << 4)) - 32;
    const int sc = static_cast<const int8_t*>(W.s2)[blk * 16 + half * 8 + kk / 16 + 2 * g];
    const float d = static_cast<const float*>(W.s)[blk];
    return __fmul_rn(__fmul_rn(d, (float)qw), (float)sc);
}

__global__ __launch_bounds__(256) void qdequant_kernel(QMat W, float* out)
{
    const int64_t total = (int64_t)W.n * W.k;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = q_element(W, i / W.k, (int)(i % W.k));
}

__global__ __launch_bounds__(256) void qembed_kernel(const uint32_t* ids, QMat table, float* out)
{
    const uint32_t id = ids[blockIdx.x];
    float* o = out + (int64_t)blockIdx.x * table.k;
    for (int c = threadIdx.x; c < table.k; c += 256) o[c] = id < (uint32_t)table.n ? q_element(table, id, c) : 0.0f;
}

}  // namespace

bool ggml_matrix_type(uint32_t type) { return type == GGML_Q8_0 || type == GGML_Q4_K || type == GGML_Q6_K; }

QPlanes repack_ggml(uint32_t type, const uint8_t* blocks, int n, int k)
{
    QPlanes p;
    const int64_t N = n;
    auto f16 = [](const uint8_t* src) {
        uint16_t h;
        std::memcpy(&h, src, 2);
        return f16_to_f32(h);
    };
    if (type == GGML_Q8_0) {
        if (k % 32) throw std::runtime_error("Q8_0 matrix with k % 32 != 0");
        const int64_t nb = N * (k / 32);
        p.plane[0].resize((size_t)nb * 32);
        p.plane[2].resize((size_t)nb * 4);
        float* s = reinterpret_cast<float*>(p.plane[2].data());
        for (int64_t b = 0; b < nb; ++b) {
            s[b] = f16(blocks + b * 34);
            std::memcpy(p.plane[0].data() + b * 32, blocks + b * 34 + 2, 32);
        }
    } else if (type == GGML_Q4_K) {
        if (k % 256) throw std::runtime_error("Q4_K matrix with k % 256 != 0");
        const int64_t nb = N * (k / 256);
        p.plane[0].resize((size_t)nb * 128);
        p.plane[2].resize((size_t)nb * 16 * 4);
        float* s = reinterpret_cast<float*>(p.plane[2].data());
        for (int64_t b = 0; b < nb; ++b) {
            const uint8_t* src = blocks + b * 144;
            const float d = f16(src), dmin = f16(src + 2);
            for (int j = 0; j < 8; ++j) {
                uint8_t sc, m;
                q4k_scale_min(j, src + 4, &sc, &m);
                s[b * 16 + j] = d * (float)sc;  // the products dequantize.rs forms
                s[b * 16 + 8 + j] = dmin * (float)m;
            }
            std::memcpy(p.plane[0].data() + b * 128, src + 16, 128);
        }
    } else if (type == GGML_Q6_K) {
        if (k % 256) throw std::runtime_error("Q6_K matrix with k % 256 != 0");
        const int64_t nb = N * (k / 256);
        p.plane[0].resize((size_t)nb * 128);
        p.plane[1].resize((size_t)nb * 64);
        p.plane[2].resize((size_t)nb * 4);
        p.plane[3].resize((size_t)nb * 16);
        float* s = reinterpret_cast<float*>(p.plane[2].data());
        for (int64_t b = 0; b < nb; ++b) {
            const uint8_t* src = blocks + b * 210;
            std::memcpy(p.plane[0].data() + b * 128, src, 128);
            std::memcpy(p.plane[1].data() + b * 64, src + 128, 64);
            std::memcpy(p.plane[3].data() + b * 16, src + 192, 16);
            s[b] = f16(src + 208);
        }
    } else {
        throw std::runtime_error(std::string("not a quantized matrix type: ") + ggml_type_name(type));
    }
    return p;
}

hipError_t launch_qfused(const QFusedArgs& a, hipStream_t stream)
{
    if (a.rows < 1 || a.rows > 8 || a.jobs < 1 || a.k % 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.jobs + kWaves - 1) / kWaves)), block(64 * kWaves);
    if (a.rows == 1) hipLaunchKernelGGL(qfused_kernel<1>, grid, block, 0, stream, a);
    else if (a.rows <= 4) hipLaunchKernelGGL(qfused_kernel<4>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(qfused_kernel<8>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_qgemv(const QGemvArgs& g, hipStream_t stream)
{
    QFusedArgs a;
    a.mode = QF_PLAIN;
    a.W[0] = g.W;
    a.seg_jobs[0] = (g.W.n + 1) / 2;
    a.jobs = a.seg_jobs[0];
    a.k = g.W.k; a.X = g.X; a.ldx = g.ldx; a.rows = g.rows; a.Xq = g.Xq; a.Xd = g.Xd; a.bias = g.bias; a.R = g.R; a.ldr = g.ldr;
    a.Y[0] = g.Y; a.ldy[0] = g.ldy;
    return launch_qfused(a, stream);
}

hipError_t launch_q8k_quantize(const float* X, int64_t ldx, int rows, int k, int8_t* codes, float* scales, float* deq, hipStream_t stream)
{
    if (k % 256 || rows < 1) return hipErrorInvalidValue;
    const int blocks = rows * (k / 256);
    hipLaunchKernelGGL(q8k_quantize_kernel, dim3((unsigned)((blocks + 3) / 4)), dim3(256), 0, stream, X, ldx, rows, k, codes, scales, deq);
    return hipGetLastError();
}

hipError_t launch_qprep(const float* X, int64_t ldx, int rows, int k, const float* gamma, float eps, float* xn, int8_t* codes, float* scales,
                        hipStream_t stream)
{
    if (k % 256 || rows < 1 || (codes && !scales)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qprep_kernel, dim3((unsigned)rows), dim3(256), 0, stream, X, ldx, k, gamma, eps, xn, codes, scales);
    return hipGetLastError();
}

hipError_t launch_qdequant(const QMat& W, float* out, hipStream_t stream)
{
    const int64_t total = (int64_t)W.n * W.k;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(qdequant_kernel, dim3(grid), dim3(256), 0, stream, W, out);
    return hipGetLastError();
}

hipError_t launch_qembed(const uint32_t* ids, int n, const QMat& table, float* out, hipStream_t stream)
{
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(qembed_kernel, dim3((unsigned)n), dim3(256), 0, stream, ids, table, out);
    return hipGetLastError();
}

}  // namespace kjarni
