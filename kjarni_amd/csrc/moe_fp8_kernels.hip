// The sparse FFN of Qwen3-MoE decoders over FP8 (OCP e4m3fn) expert stacks (moe_fp8_kernels.h): the codes and their f32 scales stay
// as they are in HBM, the matrix of a slot is chosen by an expert id read on the device.  Router, pick, plan and combine are
// moe_kernels.hip's launches; the three kernels that touch an expert matrix are here:
//   steps route (rows <= 8)   gate / up + SwiGLU and down + combine + residual as weight-streaming GEMVs: a lane reads 16 codes per
//                             16-byte non-temporal load, decodes them in hardware (fp8_decode.h) and multiplies in f32 against the
//                             row held in LDS.  LDS holds the row as four planes of quads (quad q of piece p at float4 slot
//                             q * pieces + p): the 64 lanes of a wave read 64 consecutive float4 for each quad of their pieces.
//                             Block scales multiply the sum of each 16-code piece (a piece never straddles a 128-wide block), channel
//                             and tensor scales the finished dot product -- the order of fp8_kernels.hip.
//   rows route                the grouped GEMM on v_mfma_f32_32x32x16_bf16: rows gathered through the sorted slot list and split
//                             into three exact bf16 planes in the tile loader (bf16_split.h), the codes turned into exact bf16
//                             operands there too; every product exact, f32 accumulation; block scales folded in f32 whenever K
//                             reaches a multiple of 128, channel / tensor scales in the epilogue.  gate / up: one pass over A, two
//                             weight planes, two accumulators, silu(g) * u in the epilogue.
// Compiled with -fno-slp-vectorize like the other users of bf16_split.h (the Makefile says why).
#include "moe_fp8_kernels.h"

#include "bf16_split.h"
#include "device_utils.h"
#include "fp8_decode.h"
#include "llm_kernels.h"

namespace kjarni {

namespace {

__device__ inline float silu(float g) { return g / (1.0f + expf(-g)); }
__device__ inline int clamp_expert(int e, int E) { return min(max(e, 0), E - 1); }  // (a stray id must not leave the stack)

// One stack as the kernels index it.  Scale of (expert e, row j, column i):
//   block    scale[e * per + (j >> 7) * scale_cols + (i >> 7)];   channel  scale[e * per + j];   tensor  scale[e]
struct Fp8Stk {
    const uint8_t* codes;
    const float* scale;
    int64_t per;     // floats of scale per expert
    int scale_cols;  // k / 128 for block scales, else 0
    int chan;        // 1 per channel, else 0
};

Fp8Stk make_stk(const MoeFp8Stack& s, int n, int k)
{
    Fp8Stk o;
    o.codes = s.codes;
    o.scale = s.scale;
    o.per = moe_fp8_scale_extent(s.kind, n, k);
    o.scale_cols = s.kind == FP8_BLOCK ? k / kFp8Block : 0;
    o.chan = s.kind == FP8_PER_CHANNEL ? 1 : 0;
    return o;
}

// acc (+)= the 16 products of a piece: the row's four quads x against the piece's codes.  BLOCK: the piece's own sum times its scale.
template <bool BLOCK>
__device__ __forceinline__ float piece_dot(const f32x4 (&x)[4], u32x4 raw, float sc, float acc)
{
    float w[16];
    decode16(raw, w);
    float t = BLOCK ? 0.0f : acc;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int c = 0; c < 4; ++c) t = fmaf(x[d][c], w[4 * d + c], t);
    return BLOCK ? fmaf(t, sc, acc) : t;
}

// ---- steps route ---------------------------------------------------------------------------------------------------------------------

// grid (Im / 16, rows * k), 4 waves: the workgroup of slot (row, j) reads its expert id, normalises the row into LDS once, then each
// wave streams 4 rows of that expert's gate and of its up matrix: 8 loads of 16 codes per lane in flight per step of 1 024 columns.
template <bool BLOCK>
__global__ __launch_bounds__(256) void moe_fp8_gate_up_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ gamma, float eps,
                                                              const int32_t* __restrict__ ids, int k, int E, const Fp8Stk gate, const Fp8Stk up,
                                                              int H, int Im, float* __restrict__ mid)
{
    extern __shared__ __attribute__((aligned(16))) f32x4 sx4[];  // [H / 4], quad planes
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int slot = blockIdx.y, row = slot / k;
    const int e = clamp_expert(ids[slot], E);
    const int P = H >> 4, h4 = H >> 2;  // pieces and quads of a row
    const float* x = X + (int64_t)row * ldx;
    float ss = 0.0f;
    for (int i = tid; i < h4; i += 256) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * i);
        sx4[(i & 3) * P + (i >> 2)] = xv;
#pragma unroll
        for (int c = 0; c < 4; ++c) ss = fmaf(xv[c], xv[c], ss);
    }
    if (gamma) {  // (uniform)
        ss = wave_sum(ss);
        if (lane == 0) red[wid] = ss;
        __syncthreads();
        const float rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
        for (int i = tid; i < h4; i += 256) {  // every thread rewrites what it wrote
            f32x4 xv = sx4[(i & 3) * P + (i >> 2)];
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * i);
#pragma unroll
            for (int c = 0; c < 4; ++c) xv[c] = (xv[c] / rms) * g[c];
            sx4[(i & 3) * P + (i >> 2)] = xv;
        }
    }
    __syncthreads();
    const int c0 = blockIdx.x * 16 + wid * 4;  // Im % 16 == 0: every column exists; c0 .. c0 + 3 lie in one row of blocks
    const uint8_t* g = gate.codes + ((int64_t)e * Im + c0) * H;  // 64-bit: E * Im * H passes 2^31 at the large widths
    const uint8_t* u = up.codes + ((int64_t)e * Im + c0) * H;
    const float* gs = gate.scale + (int64_t)e * gate.per + (int64_t)(c0 >> 7) * gate.scale_cols;
    const float* us = up.scale + (int64_t)e * up.per + (int64_t)(c0 >> 7) * up.scale_cols;
    float ag[4] = {0.0f, 0.0f, 0.0f, 0.0f}, au[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = lane; p < P; p += 64) {
        u32x4 rg[4], ru[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            rg[q] = load_nt16(g + (int64_t)q * H + p * 16);
            ru[q] = load_nt16(u + (int64_t)q * H + p * 16);
        }
        const float sg = BLOCK ? gs[p >> 3] : 0.0f, su = BLOCK ? us[p >> 3] : 0.0f;
        f32x4 xq[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) xq[d] = sx4[d * P + p];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ag[q] = piece_dot<BLOCK>(xq, rg[q], sg, ag[q]);
            au[q] = piece_dot<BLOCK>(xq, ru[q], su, au[q]);
        }
    }
    f32x4 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float gv = wave_sum(ag[q]), uv = wave_sum(au[q]);
        if (!BLOCK) {
            gv *= gate.scale[(int64_t)e * gate.per + (int64_t)(c0 + q) * gate.chan];
            uv *= up.scale[(int64_t)e * up.per + (int64_t)(c0 + q) * up.chan];
        }
        out[q] = silu(gv) * uv;
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(mid + (int64_t)slot * Im + c0) = out;
}

// grid (H / 16, rows), 4 waves: the row's k intermediate rows in LDS (quad planes per slot); every wave owns 4 output columns and
// walks the k slots in order, streaming 4 rows of that slot's down matrix each time.  Residual fused; one lane owns an output
// element, so R may be Y.
template <bool BLOCK>
__global__ __launch_bounds__(256) void moe_fp8_down_combine_kernel(const float* __restrict__ mid, const int32_t* __restrict__ ids,
                                                                   const float* __restrict__ weights, int k, int E, const Fp8Stk down, int H,
                                                                   int Im, const float* R, int64_t ldr, float* Y, int64_t ldy)
{
    extern __shared__ __attribute__((aligned(16))) f32x4 sm4[];  // [k][Im / 4], quad planes
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row = blockIdx.y;
    const int P = Im >> 4, i4n = Im >> 2;
    const float* m = mid + (int64_t)row * k * Im;
    for (int i = tid; i < k * i4n; i += 256) {
        const int j = i / i4n, r = i - j * i4n;
        sm4[j * i4n + (r & 3) * P + (r >> 2)] = *reinterpret_cast<const f32x4*>(m + 4 * (int64_t)i);
    }
    __syncthreads();
    const int c0 = blockIdx.x * 16 + wid * 4;  // H % 16 == 0
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < k; ++j) {
        const int e = clamp_expert(ids[row * k + j], E);
        const float wj = weights[row * k + j];
        const uint8_t* d = down.codes + ((int64_t)e * H + c0) * Im;
        const float* ds = down.scale + (int64_t)e * down.per + (int64_t)(c0 >> 7) * down.scale_cols;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int p = lane; p < P; p += 64) {
            u32x4 rd[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) rd[q] = load_nt16(d + (int64_t)q * Im + p * 16);
            const float sd = BLOCK ? ds[p >> 3] : 0.0f;
            f32x4 xq[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) xq[c] = sm4[j * i4n + c * P + p];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = piece_dot<BLOCK>(xq, rd[q], sd, a[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = wave_sum(a[q]);
            if (!BLOCK) v *= down.scale[(int64_t)e * down.per + (int64_t)(c0 + q) * down.chan];
            s[q] = fmaf(wj, v, s[q]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[(int64_t)row * ldy + c0 + q] = R[(int64_t)row * ldr + c0 + q] + s[q];
    }
}

// ---- rows route: the grouped GEMM on the codes ---------------------------------------------------------------------------------------

constexpr int QG_BM = 64, QG_BN = 64, QG_BK = 32;
constexpr int QG_PLANE = 64 * 32;  // bf16 per plane: 64 rows x 64 bytes, the four 16-byte chunks of a row swizzled by (row >> 2) & 3

// One 64 x 64 output tile of one expert (tile table of the plan): rows = up to 64 sorted slots, columns n0 .. n0 + 63 of W_e [N, K].
// 4 waves of one 32 x 32 tile each, LDS double-buffered as [stage][A1 | A2 | A3 | W (| W2)], the next step's global loads in flight
// during the MFMAs (prefill_gemm_fp8w_kernel's loop with gathered rows and a matrix chosen by the tile).
template <bool GATE_UP, int KIND>
__global__ __launch_bounds__(256) void moe_fp8_grouped_gemm_kernel(const float* __restrict__ A, int64_t lda, int a_div,
                                                                   const int32_t* __restrict__ sorted, const int32_t* __restrict__ tiles,
                                                                   const int32_t* __restrict__ ntiles, const Fp8Stk W, const Fp8Stk W2, int N,
                                                                   int K, float* __restrict__ out)
{
    constexpr int PLANES = GATE_UP ? 5 : 4;
    __shared__ __attribute__((aligned(16))) uint16_t sp[2][PLANES * QG_PLANE];
    __shared__ int s_slot[QG_BM];
    const int t = blockIdx.x;
    if (t >= *ntiles) return;  // a surplus tile (uniform, before any barrier)
    const int e = tiles[3 * t], first = tiles[3 * t + 1], cnt = tiles[3 * t + 2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.y * QG_BN;
    if (tid < QG_BM) s_slot[tid] = sorted[first + min(tid, cnt - 1)];  // rows past cnt: the last slot again, never stored
    __syncthreads();

    const int a_row = tid >> 3, a_c4 = tid & 7, b_row = tid >> 2, b_c = tid & 3;
    const float* a_ptr[2];
    int stA[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = a_row + 32 * i;
        a_ptr[i] = A + (int64_t)(s_slot[row] / a_div) * lda + a_c4 * 4;
        stA[i] = row * 32 + (((a_c4 >> 1) ^ ((row >> 2) & 3)) * 2 + (a_c4 & 1)) * 4;
    }
    const int64_t w_off = ((int64_t)e * N + min(n0 + b_row, N - 1)) * K + b_c * 8;  // 64-bit expert offset; eight codes per lane and K step
    const uint8_t* b_ptr = W.codes + w_off;
    const uint8_t* b2_ptr = GATE_UP ? W2.codes + w_off : nullptr;
    const int stW = 3 * QG_PLANE + b_row * 32 + (b_c ^ ((b_row >> 2) & 3)) * 8;
    f32x4 ga[2];
    u32x2 gw, gw2;
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
        gw = *reinterpret_cast<const u32x2*>(b_ptr + k0);
        if constexpr (GATE_UP) gw2 = *reinterpret_cast<const u32x2*>(b2_ptr + k0);
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p1, p2, p3;
            sp_split(ga[i], p1, p2, p3);
            *reinterpret_cast<u32x2*>(&sp[stage][stA[i]]) = p1;
            *reinterpret_cast<u32x2*>(&sp[stage][QG_PLANE + stA[i]]) = p2;
            *reinterpret_cast<u32x2*>(&sp[stage][2 * QG_PLANE + stA[i]]) = p3;
        }
        *reinterpret_cast<u32x4*>(&sp[stage][stW]) = fp8x8_to_bf16x8(gw);  // decoded once per element, here
        if constexpr (GATE_UP) *reinterpret_cast<u32x4*>(&sp[stage][QG_PLANE + stW]) = fp8x8_to_bf16x8(gw2);
    };
    f32x16 acc, acc2, total, total2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = total[r] = total2[r] = 0.0f;
    const int nk = K / QG_BK;
    const int fsw = (l31 >> 2) & 3;
    const int fa = (wr * 32 + l31) * 32, fb = 3 * QG_PLANE + (wc * 32 + l31) * 32;
    // (block scales: a 64-column tile starts at a multiple of 64 and so lies inside one row of blocks)
    const float* brow = W.scale + (int64_t)e * W.per + (int64_t)(n0 >> 7) * W.scale_cols;
    const float* brow2 = GATE_UP ? W2.scale + (int64_t)e * W2.per + (int64_t)(n0 >> 7) * W2.scale_cols : nullptr;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * QG_BK);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int ch = ((kb * 2 + half) ^ fsw) * 8;
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&sp[cur][fb + ch]);
            bf16x8 b2;
            if constexpr (GATE_UP) b2 = *reinterpret_cast<const bf16x8*>(&sp[cur][QG_PLANE + fb + ch]);
#pragma unroll
            for (int p = 2; p >= 0; --p) {  // the smallest piece first
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(&sp[cur][p * QG_PLANE + fa + ch]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
                if constexpr (GATE_UP) acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b2, acc2, 0, 0, 0);
            }
        }
        if (KIND == FP8_BLOCK) {
            const int k_end = (kt + 1) * QG_BK;
            if ((k_end & (kFp8Block - 1)) == 0) {  // (K % 128 == 0: the last step folds too)
                const float s = brow[(k_end - 1) >> 7];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    total[r] += s * acc[r];
                    acc[r] = 0.0f;
                }
                if constexpr (GATE_UP) {
                    const float s2 = brow2[(k_end - 1) >> 7];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        total2[r] += s2 * acc2[r];
                        acc2[r] = 0.0f;
                    }
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
            acc2 = total2;
        } else {
            const float sc = W.scale[(int64_t)e * W.per + (int64_t)col * W.chan];
            const float sc2 = GATE_UP ? W2.scale[(int64_t)e * W2.per + (int64_t)col * W2.chan] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] *= sc;
                acc2[r] *= sc2;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wr * 32 + acc_row(r, half);
            if (rr < cnt) out[(int64_t)s_slot[rr] * N + col] = GATE_UP ? silu(acc[r]) * acc2[r] : acc[r];
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool route_shape(int E, int k) { return E >= 2 && E <= MOE_MAX_EXPERTS && k >= 1 && k <= MOE_MAX_TOPK && k <= E; }
bool kind_ok(int kind) { return kind == FP8_PER_TENSOR || kind == FP8_PER_CHANNEL || kind == FP8_BLOCK; }
// a stack the kernels may read: codes 16-byte aligned (and every row of every expert with them: k % 16 == 0), block scales with k % 128 == 0
bool stack_ok(const MoeFp8Stack& s, int k) { return s.codes && s.scale && aligned16(s.codes) && kind_ok(s.kind) && k % 16 == 0 && (s.kind != FP8_BLOCK || k % kFp8Block == 0); }

}  // namespace

int64_t moe_fp8_scale_extent(int kind, int64_t n, int64_t k)
{
    if (kind == FP8_PER_TENSOR) return 1;
    if (kind == FP8_PER_CHANNEL) return n;
    if (kind == FP8_BLOCK) return (n + kFp8Block - 1) / kFp8Block * (k / kFp8Block);
    return 0;
}

hipError_t launch_moe_fp8_gate_up(const float* X, int64_t ldx, int rows, const float* gamma, float eps, const int32_t* ids, int k, int E,
                                  const MoeFp8Stack& gate, const MoeFp8Stack& up, int H, int Im, float* mid, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!route_shape(E, k) || rows > 8 || H % 32 || H < 32 || H > 8192 || Im % 32 || Im < 32 || (ldx & 3) || ldx < H || !X || !ids || !mid ||
        !aligned16(X) || !aligned16(mid) || (gamma && !aligned16(gamma)) || !stack_ok(gate, H) || !stack_ok(up, H))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(Im / 16), (unsigned)(rows * k));
    const size_t lds = (size_t)H * sizeof(float);
    const Fp8Stk g = make_stk(gate, Im, H), u = make_stk(up, Im, H);
    // one block-scaled stack: both take the per-piece form (a channel / tensor stack has scale_cols 0 and would read its first scale
    // per piece) -- the loader gives one kind per layer, the launcher refuses a mixture
    if ((gate.kind == FP8_BLOCK) != (up.kind == FP8_BLOCK)) return hipErrorInvalidValue;
    if (gate.kind == FP8_BLOCK)
        hipLaunchKernelGGL(moe_fp8_gate_up_kernel<true>, grid, dim3(256), lds, stream, X, ldx, gamma, eps, ids, k, E, g, u, H, Im, mid);
    else
        hipLaunchKernelGGL(moe_fp8_gate_up_kernel<false>, grid, dim3(256), lds, stream, X, ldx, gamma, eps, ids, k, E, g, u, H, Im, mid);
    return hipGetLastError();
}

hipError_t launch_moe_fp8_down_combine(const float* mid, int rows, const int32_t* ids, const float* weights, int k, int E,
                                       const MoeFp8Stack& down, int H, int Im, const float* R, int64_t ldr, float* Y, int64_t ldy,
                                       hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!route_shape(E, k) || rows > 8 || H % 32 || H < 32 || Im % 32 || Im < 32 || (int64_t)k * Im > 16384 || !R || !Y || !mid || !ids || !weights ||
        ldr < H || ldy < H || !aligned16(mid) || !stack_ok(down, Im))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(H / 16), (unsigned)rows);
    const size_t lds = (size_t)k * Im * sizeof(float);
    const Fp8Stk d = make_stk(down, H, Im);
    if (down.kind == FP8_BLOCK)
        hipLaunchKernelGGL(moe_fp8_down_combine_kernel<true>, grid, dim3(256), lds, stream, mid, ids, weights, k, E, d, H, Im, R, ldr, Y, ldy);
    else
        hipLaunchKernelGGL(moe_fp8_down_combine_kernel<false>, grid, dim3(256), lds, stream, mid, ids, weights, k, E, d, H, Im, R, ldr, Y, ldy);
    return hipGetLastError();
}

hipError_t launch_moe_fp8_grouped_gemm(const float* A, int64_t lda, int a_div, const int32_t* plan, int S, int E, const MoeFp8Stack& W,
                                       const MoeFp8Stack* W2, int N, int K, float* out, hipStream_t stream)
{
    if (S <= 0) return hipSuccess;
    if (E < 2 || E > MOE_MAX_EXPERTS || a_div < 1 || N < 1 || K < QG_BK || K % QG_BK || (lda & 3) || lda < K || !A || !plan || !out || !aligned16(A) ||
        !stack_ok(W, K) || (W2 && (!stack_ok(*W2, K) || (W2->kind == FP8_BLOCK) != (W.kind == FP8_BLOCK))))
        return hipErrorInvalidValue;
    const MoePlan p = moe_plan_at(const_cast<int32_t*>(plan), S, E);
    const dim3 grid((unsigned)moe_max_tiles(S, E), (unsigned)((N + QG_BN - 1) / QG_BN));
    const Fp8Stk w = make_stk(W, N, K), w2 = W2 ? make_stk(*W2, N, K) : w;
#define KJ_QG(GU, KIND)                                                                                                                    \
    hipLaunchKernelGGL((moe_fp8_grouped_gemm_kernel<GU, KIND>), grid, dim3(256), 0, stream, A, lda, a_div, p.sorted, p.tiles, p.ntiles, w, \
                       w2, N, K, out)
#define KJ_QG_KIND(KIND)            \
    do {                            \
        if (W2) KJ_QG(true, KIND);  \
        else KJ_QG(false, KIND);    \
    } while (0)
    if (W.kind == FP8_BLOCK) KJ_QG_KIND(FP8_BLOCK);
    else KJ_QG_KIND(FP8_PER_CHANNEL);  // (per tensor: the same instance, the scale's column stride is then 0)
#undef KJ_QG_KIND
#undef KJ_QG
    return hipGetLastError();
}

const char* moe_fp8_ffn_refusal(const MoeFp8FfnArgs& a, bool grouped)
{
    if (const char* why = moe_ffn_refusal(a.base, grouped)) return why;
    if (!kind_ok(a.gate.kind) || !kind_ok(a.up.kind) || !kind_ok(a.down.kind)) return "a scale kind must be 0 (per tensor), 1 (per channel) or 2 (block)";
    if ((a.gate.kind == FP8_BLOCK) != (a.up.kind == FP8_BLOCK)) return "gate and up must both carry block scales, or neither";
    if (a.gate.kind == FP8_BLOCK && a.base.H % kFp8Block) return "block scales of gate / up need hidden a multiple of 128";
    if (a.down.kind == FP8_BLOCK && a.base.Im % kFp8Block) return "block scales of down need Im a multiple of 128";
    return nullptr;
}

hipError_t launch_moe_fp8_ffn_steps(const MoeFp8FfnArgs& f, hipStream_t stream)
{
    const MoeFfnArgs& a = f.base;
    if (a.rows <= 0) return hipSuccess;
    if (moe_fp8_ffn_refusal(f, false)) return hipErrorInvalidValue;
    LlmGemvArgs g;
    g.X = a.X; g.ldx = a.ldx; g.rows = a.rows; g.gamma = a.gamma; g.eps = a.eps; g.W = a.router; g.bf16 = a.bf16; g.n_out = a.E; g.k = a.H;
    g.Y0 = a.logits; g.ldy0 = a.E;
    hipError_t e = launch_llm_gemv(g, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_route(a.logits, a.E, a.rows, a.E, a.k, a.norm_topk, a.ids, a.weights, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_fp8_gate_up(a.X, a.ldx, a.rows, a.gamma, a.eps, a.ids, a.k, a.E, f.gate, f.up, a.H, a.Im, a.mid, stream);
    if (e != hipSuccess) return e;
    return launch_moe_fp8_down_combine(a.mid, a.rows, a.ids, a.weights, a.k, a.E, f.down, a.H, a.Im, a.R, a.ldr, a.Y, a.ldy, stream);
}

hipError_t launch_moe_fp8_ffn_grouped(const MoeFp8FfnArgs& f, hipStream_t stream)
{
    const MoeFfnArgs& a = f.base;
    if (a.rows <= 0) return hipSuccess;
    if (moe_fp8_ffn_refusal(f, true)) return hipErrorInvalidValue;
    const float* x = a.X;
    int64_t ldx = a.ldx;
    hipError_t e;
    if (a.gamma) {
        e = launch_rmsnorm(a.X, a.gamma, a.eps, a.rows, a.H, a.xn, stream);
        if (e != hipSuccess) return e;
        x = a.xn;
        ldx = a.H;
    }
    e = launch_prefill_gemm(x, ldx, a.router, a.bf16, nullptr, nullptr, 0, a.logits, a.E, a.rows, a.E, a.H, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_route(a.logits, a.E, a.rows, a.E, a.k, a.norm_topk, a.ids, a.weights, stream);
    if (e != hipSuccess) return e;
    const int S = a.rows * a.k;
    e = launch_moe_group(a.ids, S, a.E, a.plan, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_fp8_grouped_gemm(x, ldx, a.k, a.plan, S, a.E, f.gate, &f.up, a.Im, a.H, a.mid, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_fp8_grouped_gemm(a.mid, a.Im, 1, a.plan, S, a.E, f.down, nullptr, a.H, a.Im, a.y, stream);
    if (e != hipSuccess) return e;
    return launch_moe_combine(a.y, a.weights, a.rows, a.k, a.H, a.R, a.ldr, a.Y, a.ldy, stream);
}

}  // namespace kjarni
