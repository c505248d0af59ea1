// FP8 (OCP e4m3fn) weights kept as their codes in HBM: the decode-step projection over 1-8 activation rows, and the
// dequantization into the prompt route's f32 scratch.  w[j, i] = decode(code[j, i]) * scale, f32 activations x dequantized
// weights with f32 accumulation (weight-only: the arithmetic of the Q8_0 / Q4_K linears of quant_kernels.hip).
//
// gfx950 decodes e4m3fn in hardware: __builtin_amdgcn_cvt_pk_f32_fp8 (v_cvt_pk_f32_fp8) turns two codes of a dword into two
// floats, exactly.  A weight therefore costs half a conversion and one FMA per row; the scale is applied once per 16-code piece
// (block scales: a piece never straddles a 128-wide block, 16 | 128) or once per output (per channel, per tensor).
//
// The projection is llm_gemv_lanes_kernel's design on one-byte weights:
//   * a workgroup (4 waves) holds a K-slice of every row in LDS, [rows][2 048] f32 (64 KB at 8 rows: two workgroups per CU), the
//     rows RMS-normalised on the way in.  K <= 2 048: staged once, the workgroup loops over batches of columns.  K > 2 048 (the
//     down projection): the slices are staged one after the other, the accumulators stay in registers, the grid covers the columns.
//     Nothing assumes that 8 rows of K floats fit in LDS.
//   * per (batch, slice) a wave owns CPW columns and each lane two 16-code pieces of each: CPW x 2 (x 2 with the SwiGLU pair)
//     non-temporal 16-byte loads per lane, all issued before the first FMA and re-issued for the next (batch, slice) before the
//     cross-lane sums of this one.
//   * LDS holds a slice as four planes of quads: quad q of piece p at float4 slot q * (pieces per slice) + p, so that the 64 lanes
//     of a wave read 64 consecutive float4 (no bank conflicts) for each of the four quads of their piece.
//   * one row (the decode step) has instances of its own: one column per wave in 62-84 VGPRs (6-8 waves per SIMD resident, against
//     2-3 of the 8-row instances), and for K > 2 048 a slice of 8 192 columns (32 KB), so that the down projection of the 1B shape
//     is one slice with eight loads per lane in flight instead of four slices with a barrier between them.
#include <algorithm>

#include "device_utils.h"
#include "dynamic_lds.h"
#include "fp8_kernels.h"

namespace kjarni {

namespace {

constexpr int F8_ROWS_LIMIT = 8;
// CH 16-code pieces per lane, column and slice: a workgroup holds CH * 1024 columns of K at a time (CH * 64 pieces per row, CH
// float4 of one row's slice per thread).

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

// One matrix as the kernels index it: scale of (row j, column i) = scale[(j >> row_shift) * scale_cols + (i >> 7) * col_mul].
struct Fp8Seg {
    const uint8_t* codes;
    const float* scale;
    int n;
    int row_shift;   // 0 per channel, 7 block, 31 per tensor
    int scale_cols;  // k / 128 for block scales, else 1
    int col_mul;     // 1 for block scales, else 0
};

struct Fp8KArgs {
    Fp8Seg seg[3];
    int n_tot, k, rows;
    const float* X;
    int64_t ldx;
    const float* gamma;
    float eps;
    const float* bias;
    const float* R;
    int64_t ldr;
    float* Y0;
    float* Y1;
    float* Y2;
    int64_t ldy0, ldy1, ldy2;
    int row_off;
    const int* row_off_ptr;
};

Fp8Seg make_seg(const Fp8Mat& m)
{
    Fp8Seg s;
    s.codes = m.codes;
    s.scale = m.scale;
    s.n = m.n;
    s.row_shift = m.kind == FP8_BLOCK ? 7 : (m.kind == FP8_PER_CHANNEL ? 0 : 31);
    s.scale_cols = m.kind == FP8_BLOCK ? m.k / kFp8Block : 1;
    s.col_mul = m.kind == FP8_BLOCK ? 1 : 0;
    return s;
}

__device__ __forceinline__ u32x4 load_nt16(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }

// The 16 codes of a piece as floats (code 4 d + e of the piece in w[4 d + e]).
__device__ __forceinline__ void decode16(u32x4 p, float (&w)[16])
{
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const f32x2v lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)p[d], false);
        const f32x2v hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)p[d], true);
        w[4 * d] = lo[0];
        w[4 * d + 1] = lo[1];
        w[4 * d + 2] = hi[0];
        w[4 * d + 3] = hi[1];
    }
}

// Column n of the concatenated matrices: which segment, and its row there (NM == 2: both segments hold column n).
__device__ __forceinline__ void locate(const Fp8KArgs& a, int n, int& which, int& local)
{
    which = 0;
    local = n;
    if (n >= a.seg[0].n) {
        which = 1;
        local = n - a.seg[0].n;
        if (local >= a.seg[1].n) {
            which = 2;
            local -= a.seg[1].n;
        }
    }
}

// NM: matrices per output (2: the SwiGLU pair seg[0] = gate, seg[1] = up); NORM: RMSNorm of the rows; BLOCK: a scale per piece
// (else per output, applied after the sum); CPW: columns per wave and batch; MAXR: the most rows (1: the decode step, whose
// registers then allow the occupancy that keeps a whole slice of the matrix in flight; 8); CH: pieces per lane and slice (2; 8
// with MAXR == 1 for K > 2 048, one slice up to K = 8 192).
template <int NM, bool NORM, bool BLOCK, int CPW, int MAXR, int CH>
__global__ __launch_bounds__(256) void fp8_proj_kernel(const Fp8KArgs a)
{
    constexpr int F8_CH = CH, F8_SLICE = CH * 1024, F8_PIECES = F8_SLICE / 16, F8_XV = CH, F8_MAX_ROWS = MAXR;
    extern __shared__ __attribute__((aligned(16))) float f8_xs[];  // [rows][F8_SLICE], quad planes (see the top of the file)
    __shared__ float st_rms[8];
    // the cache row of a captured step is read from memory, here, on every replay
    const int64_t r0 = a.row_off_ptr ? *a.row_off_ptr : a.row_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k, rows = a.rows, n_tot = a.n_tot;
    const int ns = (k + F8_SLICE - 1) / F8_SLICE;
    const int nbatches = (n_tot + 4 * CPW - 1) / (4 * CPW);

    f32x4 xv[F8_MAX_ROWS][F8_XV], gv[F8_XV];
    auto load_x = [&](int s) {
#pragma unroll
        for (int j = 0; j < F8_XV; ++j) {
            const int slot = tid + j * 256, q = slot / F8_PIECES, p = slot % F8_PIECES;
            const int col = s * F8_SLICE + p * 16 + q * 4;
            const bool in = col < k;
            gv[j] = (NORM && in) ? *reinterpret_cast<const f32x4*>(a.gamma + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < F8_MAX_ROWS; ++r)
                xv[r][j] = (r < rows && in) ? *reinterpret_cast<const f32x4*>(a.X + r * a.ldx + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_x = [&]() {
#pragma unroll
        for (int r = 0; r < F8_MAX_ROWS; ++r) {
            if (r < rows) {
#pragma unroll
                for (int j = 0; j < F8_XV; ++j) {
                    f32x4 v = xv[r][j];
                    if (NORM) {
                        const float rms = st_rms[r];
#pragma unroll
                        for (int c = 0; c < 4; ++c) v[c] = (v[c] / rms) * gv[j][c];  // (past K: gamma = 0)
                    }
                    *reinterpret_cast<f32x4*>(f8_xs + r * F8_SLICE + (tid + j * 256) * 4) = v;
                }
            }
        }
    };
    u32x4 raw[NM][CPW][F8_CH];
    float psc[NM][CPW][F8_CH];
    auto issue = [&](int nb, int s) {
        const int n0 = (nb * 4 + wave) * CPW;
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int cc = 0; cc < CPW; ++cc) {
                const int n = n0 + cc < n_tot ? n0 + cc : n_tot - 1;
                int which = m, local = n;
                if (NM == 1) locate(a, n, which, local);
                const Fp8Seg& sg = a.seg[which];
                const uint8_t* row = sg.codes + (int64_t)local * k;
#pragma unroll
                for (int c = 0; c < F8_CH; ++c) {
                    int e = s * F8_SLICE + (c * 64 + lane) * 16;
                    e = e < k ? e : 0;  // a piece past K reads piece 0 again and meets zeros in LDS
                    raw[m][cc][c] = load_nt16(row + e);
                    if (BLOCK) psc[m][cc][c] = sg.scale[(int64_t)(local >> sg.row_shift) * sg.scale_cols + (e >> 7) * sg.col_mul];
                }
            }
    };

    int nb = blockIdx.x, s = 0;
    load_x(0);
    issue(nb, 0);
    if (NORM) {  // the rms of each whole row, one wave per row (the loads above are in flight meanwhile)
        const int k4 = k >> 2;
        for (int r = wave; r < rows; r += 4) {
            const float* xr = a.X + r * a.ldx;
            float acc = 0.0f;
            for (int i = lane; i < k4; i += 64) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(xr + i * 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fmaf(x[c], x[c], acc);
            }
            const float rms = sqrtf(wave_sum(acc) / (float)k + a.eps);
            if (lane == 0) st_rms[r] = rms;
        }
        __syncthreads();
    }

    float acc[NM][CPW][F8_MAX_ROWS];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int cc = 0; cc < CPW; ++cc)
#pragma unroll
            for (int r = 0; r < F8_MAX_ROWS; ++r) acc[m][cc][r] = 0.0f;
    bool first = true;
    for (;;) {
        if (first || ns > 1) {
            if (!first) __syncthreads();  // every wave is done with the slice in LDS
            store_x();
            __syncthreads();
        }
        first = false;
#pragma unroll
        for (int c = 0; c < F8_CH; ++c) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float w[CPW][16];
#pragma unroll
                for (int cc = 0; cc < CPW; ++cc) decode16(raw[m][cc][c], w[cc]);
#pragma unroll
                for (int r = 0; r < F8_MAX_ROWS; ++r) {
                    if (r < rows) {
                        f32x4 x[4];
#pragma unroll
                        for (int d = 0; d < 4; ++d)
                            x[d] = *reinterpret_cast<const f32x4*>(f8_xs + r * F8_SLICE + (d * F8_PIECES + c * 64 + lane) * 4);
#pragma unroll
                        for (int cc = 0; cc < CPW; ++cc) {
                            float t = BLOCK ? 0.0f : acc[m][cc][r];
#pragma unroll
                            for (int d = 0; d < 4; ++d)
#pragma unroll
                                for (int e = 0; e < 4; ++e) t = fmaf(x[d][e], w[cc][4 * d + e], t);
                            acc[m][cc][r] = BLOCK ? fmaf(t, psc[m][cc][c], acc[m][cc][r]) : t;
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
                for (int r = 0; r < F8_MAX_ROWS; ++r) {
                    if (r < rows) {
                        const float t = wave_sum(acc[0][cc][r]);
                        mine = lane == r ? t : mine;
                        if (NM == 2) {
                            const float t2 = wave_sum(acc[NM - 1][cc][r]);
                            mine2 = lane == r ? t2 : mine2;
                        }
                    }
#pragma unroll
                    for (int m = 0; m < NM; ++m) acc[m][cc][r] = 0.0f;
                }
                const int n = n0 + cc;
                if (lane < rows && n < n_tot) {
                    int which = 0, local = n;
                    if (NM == 1) locate(a, n, which, local);
                    if (!BLOCK) {
                        mine *= a.seg[which].scale[local >> a.seg[which].row_shift];
                        if (NM == 2) mine2 *= a.seg[1].scale[local >> a.seg[1].row_shift];
                    }
                    float v = mine + (a.bias ? a.bias[n] : 0.0f);
                    if (NM == 2) v = (v / (1.0f + expf(-v))) * mine2;  // silu(gate) * up
                    if (a.R) v += a.R[lane * a.ldr + n];
                    float* Y = which == 0 ? a.Y0 : (which == 1 ? a.Y1 : a.Y2);
                    const int64_t ldy = which == 0 ? a.ldy0 : (which == 1 ? a.ldy1 : a.ldy2);
                    Y[((which == 0 ? 0 : r0) + lane) * ldy + local] = v;
                }
            }
        }
        if (!more) break;
        s = s2;
        nb = nb2;
    }
}

// out[j, i] = decode(code[j, i]) * scale(j, i): a thread per 16-code piece.
__global__ __launch_bounds__(256) void fp8_dequant_kernel(const Fp8Seg w, int k, int64_t pieces, float* __restrict__ out)
{
    const int ppr = k >> 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pieces; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / ppr;
        const int e = (int)(i - row * ppr) * 16;
        const u32x4 p = *reinterpret_cast<const u32x4*>(w.codes + row * k + e);
        const float sc = w.scale[(row >> w.row_shift) * w.scale_cols + (e >> 7) * w.col_mul];
        float v[16];
        decode16(p, v);
        float* o = out + row * k + e;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            *reinterpret_cast<f32x4*>(o + 4 * d) = f32x4{v[4 * d] * sc, v[4 * d + 1] * sc, v[4 * d + 2] * sc, v[4 * d + 3] * sc};
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int NM, bool NORM>
hipError_t launch_proj_t(const Fp8KArgs& k, bool block, hipStream_t stream)
{
    const bool one = k.rows == 1;
    const int ch = one && k.k > 2048 ? 8 : 2;
    const int slice = ch * 1024;
    const int ns = (k.k + slice - 1) / slice;
    // several rows: four columns per wave (8 or 16 loads per lane in flight) where that still leaves two workgroups for every CU;
    // one row: one column per wave, whose 62-84 VGPRs let 6-8 waves per SIMD stay resident
    constexpr int kWide = 4;
    const bool wide = !one && (k.n_tot + 4 * kWide - 1) / (4 * kWide) >= 512;
    const int cpw = wide ? kWide : 1;
    const int nbatches = (k.n_tot + 4 * cpw - 1) / (4 * cpw);
    // one slice: the rows stay in LDS and the workgroup loops over its batches; several: the grid covers the columns
    // (one row, measured on the Llama-1B shape: 0.803 / 0.761 / 0.714 / 0.707 / 0.749 ms per token at 256 / 384 / 512 / 768 / 2 048
    // workgroups, and 0.728 with four columns per wave)
    const int wgs = ns == 1 ? std::min(nbatches, one ? 768 : 512) : nbatches;
    const size_t lds = (size_t)k.rows * slice * sizeof(float);
#define KJ_F8_LAUNCH3(BLOCK, CPW, MAXR, CH)                                                  \
    do {                                                                                     \
        auto kern = fp8_proj_kernel<NM, NORM, BLOCK, CPW, MAXR, CH>;                         \
        if (lds > 48 * 1024) {                                                               \
            const hipError_t e = allow_dynamic_lds(kern, lds);                               \
            if (e != hipSuccess) return e;                                                   \
        }                                                                                    \
        hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), lds, stream, k);            \
    } while (0)
#define KJ_F8_LAUNCH(BLOCK)                                                                  \
    do {                                                                                     \
        if (ch == 8) KJ_F8_LAUNCH3(BLOCK, 1, 1, 8);                                          \
        else if (one) KJ_F8_LAUNCH3(BLOCK, 1, 1, 2);                                         \
        else if (wide) KJ_F8_LAUNCH3(BLOCK, kWide, 8, 2);                                    \
        else KJ_F8_LAUNCH3(BLOCK, 1, 8, 2);                                                  \
    } while (0)
    if (block) KJ_F8_LAUNCH(true);
    else KJ_F8_LAUNCH(false);
#undef KJ_F8_LAUNCH
#undef KJ_F8_LAUNCH3
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fp8_proj(const Fp8ProjArgs& a, hipStream_t stream)
{
    const int nmat = a.mode == F8_QKV ? 3 : (a.mode == F8_SWIGLU ? 2 : 1);
    if (a.mode != F8_PLAIN && a.mode != F8_QKV && a.mode != F8_SWIGLU) return hipErrorInvalidValue;
    if (a.rows < 1 || a.rows > F8_ROWS_LIMIT || !a.X || (a.ldx & 3) || !aligned16(a.X) || (a.gamma && !aligned16(a.gamma))) return hipErrorInvalidValue;
    const int k = a.W[0].k;
    if (k <= 0 || k % 16) return hipErrorInvalidValue;
    Fp8KArgs g{};
    bool block = false;
    int n_tot = 0;
    for (int i = 0; i < nmat; ++i) {
        const Fp8Mat& m = a.W[i];
        if (m.k != k || m.n <= 0 || !m.codes || !m.scale || !aligned16(m.codes) || (m.kind == FP8_BLOCK && k % kFp8Block)) return hipErrorInvalidValue;
        if (m.kind != FP8_PER_TENSOR && m.kind != FP8_PER_CHANNEL && m.kind != FP8_BLOCK) return hipErrorInvalidValue;
        g.seg[i] = make_seg(m);
        block = block || m.kind == FP8_BLOCK;
        n_tot += m.n;
    }
    for (int i = nmat; i < 3; ++i) {  // (never selected: locate() stops at the segments that exist)
        g.seg[i] = g.seg[0];
        g.seg[i].n = 0x3fffffff;
    }
    if (a.mode == F8_SWIGLU) {
        if (a.W[1].n != a.W[0].n || !a.gamma || a.R) return hipErrorInvalidValue;
        n_tot = a.W[0].n;
    }
    if (a.mode == F8_PLAIN) g.seg[0].n = 0x3fffffff;  // every column is segment 0's
    if (a.R && a.gamma) return hipErrorInvalidValue;
    for (int i = 0; i < (a.mode == F8_QKV ? 3 : 1); ++i)
        if (!a.Y[i]) return hipErrorInvalidValue;
    g.n_tot = n_tot; g.k = k; g.rows = a.rows; g.X = a.X; g.ldx = a.ldx; g.gamma = a.gamma; g.eps = a.eps; g.bias = a.bias; g.R = a.R; g.ldr = a.ldr;
    g.Y0 = a.Y[0]; g.Y1 = a.Y[1]; g.Y2 = a.Y[2]; g.ldy0 = a.ldy[0]; g.ldy1 = a.ldy[1]; g.ldy2 = a.ldy[2];
    g.row_off = a.row_off; g.row_off_ptr = a.row_off_ptr;
    if (a.mode == F8_SWIGLU) return launch_proj_t<2, true>(g, block, stream);
    return a.gamma ? launch_proj_t<1, true>(g, block, stream) : launch_proj_t<1, false>(g, block, stream);
}

hipError_t launch_fp8_dequant(const Fp8Mat& W, float* out, hipStream_t stream)
{
    if (W.n <= 0 || W.k <= 0 || W.k % 16 || !W.codes || !W.scale || !out || !aligned16(W.codes) || !aligned16(out) ||
        (W.kind == FP8_BLOCK && W.k % kFp8Block))
        return hipErrorInvalidValue;
    const int64_t pieces = (int64_t)W.n * (W.k / 16);
    const unsigned blocks = (unsigned)std::min<int64_t>((pieces + 255) / 256, 8192);
    hipLaunchKernelGGL(fp8_dequant_kernel, dim3(blocks), dim3(256), 0, stream, make_seg(W), W.k, pieces, out);
    return hipGetLastError();
}

}  // namespace kjarni
