// The sparse FFN of Qwen3-MoE decoders (moe_kernels.h): the router pick, the expert projections of the steps route (weight-
// streaming GEMVs over a stack indexed by a device-held expert id), and the rows route (device counting sort of the slots by
// expert, a grouped matrix-core GEMM over the sorted rows, an ordered combine).  No float atomics; every sum has one order.
#include "moe_kernels.h"

#include <algorithm>

#include "llm_kernels.h"

namespace kjarni {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline int wave_sum_int(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline float silu(float g) { return g / (1.0f + expf(-g)); }
__device__ inline int clamp_expert(int e, int E) { return min(max(e, 0), E - 1); }  // (ids come from moe_route_kernel; a stray one must not leave the stack)

// eight consecutive weights as f32; a bf16 is the upper half of the f32 with the same value, so a shift is exact
__device__ inline void load8(const float* p, float (&w)[8])
{
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        w[c] = a[c];
        w[4 + c] = b[c];
    }
}
__device__ inline void load8(const uint16_t* p, float (&w)[8])
{
    const u32x4 q = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        w[2 * c] = __uint_as_float(q[c] << 16);
        w[2 * c + 1] = __uint_as_float(q[c] & 0xFFFF0000u);
    }
}

// ---- the router pick ---------------------------------------------------------------------------------------------------------------

// floats as unsigned keys of the same order (NaN counts as -inf, -0 as +0), the expert below them so that the lower index wins a tie
__device__ inline unsigned long long route_key(float v, int e)
{
    v = v == v ? v + 0.0f : -INFINITY;
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)e);
}

// One wave per row, E <= 256 is four logits per lane.  k rounds of a wave-wide arg-max over the keys; the chosen expert's
// probability is exp(r - max) / sum, the renormalised weight exp(r - max) / (the k chosen exponentials, added in slot order).
__global__ __launch_bounds__(256) void moe_route_kernel(const float* __restrict__ logits, int64_t ldl, int rows, int E, int k, int norm_topk,
                                                        int32_t* __restrict__ ids, float* __restrict__ weights)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;  // (uniform per wave; no barrier below)
    const float* r = logits + (int64_t)row * ldl;
    float v[4];
    unsigned long long key[4];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        v[i] = e < E ? r[e] : -INFINITY;
        key[i] = e < E ? route_key(v[i], e) : 0ull;
        mx = fmaxf(mx, v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) part += lane + 64 * i < E ? expf(v[i] - mx) : 0.0f;
    const float sum = wave_sum(part);
    float ksum = 0.0f, mine = 0.0f;
    int my_id = 0;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = key[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) best = key[i] > best ? key[i] : best;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        const int e = min((int)(0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull)), E - 1);  // (k <= E: a live key every round)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (lane + 64 * i == e) key[i] = 0ull;
        const float pe = expf(r[e] - mx);
        ksum += pe;
        if (lane == j) {
            mine = pe;
            my_id = e;
        }
    }
    if (lane < k) {
        ids[(int64_t)row * k + lane] = my_id;
        weights[(int64_t)row * k + lane] = mine / (norm_topk ? ksum : sum);
    }
}

// ---- steps route: rows <= 8 ----------------------------------------------------------------------------------------------------------

// grid (Im / 16, rows * k): the workgroup of slot (row, j) reads its expert id first, in plain C++, then streams 16 rows of that
// expert's gate and up matrices (4 per wave, 16-byte loads) against the activation row held in LDS (normalised here when gamma).
template <typename WT>
__global__ __launch_bounds__(256) void moe_gate_up_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ gamma, float eps,
                                                          const int32_t* __restrict__ ids, int k, int E, const WT* __restrict__ gate,
                                                          const WT* __restrict__ up, int H, int Im, float* __restrict__ mid)
{
    extern __shared__ __attribute__((aligned(16))) float sx[];  // [H]
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int slot = blockIdx.y, row = slot / k;
    const int e = clamp_expert(ids[slot], E);
    const float* x = X + (int64_t)row * ldx;
    float ss = 0.0f;
    for (int i = tid * 4; i < H; i += 1024) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
        *reinterpret_cast<f32x4*>(sx + i) = xv;
#pragma unroll
        for (int c = 0; c < 4; ++c) ss = fmaf(xv[c], xv[c], ss);
    }
    if (gamma) {  // (uniform)
        ss = wave_sum(ss);
        if (lane == 0) red[wid] = ss;
        __syncthreads();
        const float rms = sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
        for (int i = tid * 4; i < H; i += 1024) {  // every thread rewrites what it wrote
            f32x4 xv = *reinterpret_cast<const f32x4*>(sx + i);
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + i);
#pragma unroll
            for (int c = 0; c < 4; ++c) xv[c] = (xv[c] / rms) * g[c];
            *reinterpret_cast<f32x4*>(sx + i) = xv;
        }
    }
    __syncthreads();
    const int c0 = blockIdx.x * 16 + wid * 4;  // Im % 16 == 0: every column exists
    const WT* g = gate + ((int64_t)e * Im + c0) * H;  // 64-bit: E * Im * H passes 2^31 at the large widths
    const WT* u = up + ((int64_t)e * Im + c0) * H;
    float ag[4] = {0.0f, 0.0f, 0.0f, 0.0f}, au[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane * 8; i < H; i += 512) {
        float xv[8], w[8];
        load8(sx + i, xv);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            load8(g + (int64_t)q * H + i, w);
#pragma unroll
            for (int c = 0; c < 8; ++c) ag[q] = fmaf(w[c], xv[c], ag[q]);
            load8(u + (int64_t)q * H + i, w);
#pragma unroll
            for (int c = 0; c < 8; ++c) au[q] = fmaf(w[c], xv[c], au[q]);
        }
    }
    f32x4 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = silu(wave_sum(ag[q])) * wave_sum(au[q]);
    if (lane == 0) *reinterpret_cast<f32x4*>(mid + (int64_t)slot * Im + c0) = out;
}

// grid (H / 8, rows): the row's k intermediate rows in LDS; every wave owns 2 output columns and walks the k slots in order,
// streaming 2 rows of that slot's down matrix each time.  Residual fused; one lane owns an output element, so R may be Y.
template <typename WT>
__global__ __launch_bounds__(256) void moe_down_combine_kernel(const float* __restrict__ mid, const int32_t* __restrict__ ids,
                                                               const float* __restrict__ weights, int k, int E, const WT* __restrict__ down,
                                                               int H, int Im, const float* R, int64_t ldr, float* Y, int64_t ldy)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];  // [k, Im]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row = blockIdx.y;
    const float* m = mid + (int64_t)row * k * Im;
    for (int i = tid * 4; i < k * Im; i += 1024) *reinterpret_cast<f32x4*>(sm + i) = *reinterpret_cast<const f32x4*>(m + i);
    __syncthreads();
    const int c0 = blockIdx.x * 8 + wid * 2;  // H % 8 == 0
    float s[2] = {0.0f, 0.0f};
    for (int j = 0; j < k; ++j) {
        const int e = clamp_expert(ids[row * k + j], E);
        const float wj = weights[row * k + j];
        const WT* d = down + ((int64_t)e * H + c0) * Im;
        float a[2] = {0.0f, 0.0f};
        for (int i = lane * 8; i < Im; i += 512) {
            float xv[8], w[8];
            load8(sm + j * Im + i, xv);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                load8(d + (int64_t)q * Im + i, w);
#pragma unroll
                for (int c = 0; c < 8; ++c) a[q] = fmaf(w[c], xv[c], a[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) s[q] = fmaf(wj, wave_sum(a[q]), s[q]);
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) Y[(int64_t)row * ldy + c0 + q] = R[(int64_t)row * ldr + c0 + q] + s[q];
    }
}

// ---- rows route: the plan ------------------------------------------------------------------------------------------------------------

// One wave per expert counts its slots.
__global__ __launch_bounds__(64) void moe_count_kernel(const int32_t* __restrict__ ids, int S, int32_t* __restrict__ counts)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    int c = 0;
    for (int s = lane; s < S; s += 64) c += ids[s] == e ? 1 : 0;
    c = wave_sum_int(c);
    if (lane == 0) counts[e] = c;
}

// One wave per expert: its offset and first tile from the counts before it, its tiles, then its slots in slot order (a stable
// counting sort by ballot: no atomics, the same list every run).
__global__ __launch_bounds__(64) void moe_place_kernel(const int32_t* __restrict__ ids, int S, int E, const int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ sorted, int32_t* __restrict__ offsets, int32_t* __restrict__ tiles,
                                                       int32_t* __restrict__ ntiles)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    int off = 0, tb = 0;
    for (int i = lane; i < e; i += 64) {
        const int c = counts[i];
        off += c;
        tb += (c + MOE_TILE_ROWS - 1) / MOE_TILE_ROWS;
    }
    off = wave_sum_int(off);
    tb = wave_sum_int(tb);
    const int mine = counts[e], my_tiles = (mine + MOE_TILE_ROWS - 1) / MOE_TILE_ROWS;
    if (lane == 0) {
        offsets[e] = off;
        if (e == E - 1) {
            offsets[E] = off + mine;
            *ntiles = tb + my_tiles;
        }
    }
    for (int t = lane; t < my_tiles; t += 64) {
        tiles[3 * (tb + t) + 0] = e;
        tiles[3 * (tb + t) + 1] = off + MOE_TILE_ROWS * t;
        tiles[3 * (tb + t) + 2] = min(MOE_TILE_ROWS, mine - MOE_TILE_ROWS * t);
    }
    int base = off;
    const int end = off + mine;  // (the ids do not change between the two kernels; the bound holds whatever they are)
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool hit = s < S && ids[s] == e;
        const unsigned long long b = __ballot(hit);
        const int at = base + __popcll(b & ((1ull << lane) - 1ull));
        if (hit && at < end) sorted[at] = s;
        base += __popcll(b);
    }
}

// ---- rows route: the grouped GEMM ----------------------------------------------------------------------------------------------------

constexpr int MG_BM = 64, MG_BN = 64, MG_BK = 32, MG_STRIDE = MG_BK + 4;

__device__ inline int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }  // row of accumulator register r (32 x 32 MFMA)

// One 64 x 64 output tile of one expert: rows = up to 64 sorted slots (tile table), columns n0 .. n0 + 63 of W_e [N, K].
// prefill_gemm_kernel's design: 4 waves, one 32 x 32 MFMA tile each, BK = 32, operands double-buffered in LDS with the next
// tile's global loads in flight during the MFMAs.  A rows are gathered: row of sorted slot s is s / a_div.  GATE_UP: a second
// weight tile (up) and accumulator, epilogue silu(gate) * up.  Output rows are slot-major: out[slot, N].
template <typename WT, bool GATE_UP>
__global__ __launch_bounds__(256) void moe_grouped_gemm_kernel(const float* __restrict__ A, int64_t lda, int a_div,
                                                               const int32_t* __restrict__ sorted, const int32_t* __restrict__ tiles,
                                                               const int32_t* __restrict__ ntiles, const WT* __restrict__ W,
                                                               const WT* __restrict__ W2, int N, int K, float* __restrict__ out)
{
    constexpr bool BF = sizeof(WT) == 2;
    __shared__ __attribute__((aligned(16))) float sA[2][MG_BM * MG_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB[2][MG_BN * MG_STRIDE];
    __shared__ __attribute__((aligned(16))) float sB2[GATE_UP ? 2 : 1][GATE_UP ? MG_BN * MG_STRIDE : 4];
    __shared__ int s_slot[MG_BM];
    const int t = blockIdx.x;
    if (t >= *ntiles) return;  // a surplus tile (uniform, before any barrier)
    const int e = tiles[3 * t], first = tiles[3 * t + 1], cnt = tiles[3 * t + 2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, l31 = lane & 31, half = lane >> 5;
    const int n0 = blockIdx.y * MG_BN;
    if (tid < MG_BM) s_slot[tid] = sorted[first + min(tid, cnt - 1)];
    __syncthreads();

    const int a_row = tid >> 3, a_c4 = tid & 7;
    const float* a_ptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a_ptr[i] = A + (int64_t)(s_slot[a_row + 32 * i] / a_div) * lda + a_c4 * 4;
    const WT* We = W + (int64_t)e * N * K;  // 64-bit expert offset
    const WT* We2 = GATE_UP ? W2 + (int64_t)e * N * K : nullptr;
    // f32: 64 x 32 floats = 512 float4, two per thread (rows a_row, a_row + 32); bf16: 64 x 32 halves = 256 x 16 bytes, one per thread
    const int b_row = BF ? tid >> 2 : a_row, b_c = BF ? (tid & 3) * 8 : a_c4 * 4;
    const WT* b_ptr[2];
    const WT* b2_ptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        b_ptr[i] = We + (int64_t)min(n0 + b_row + 32 * i, N - 1) * K + b_c;
        b2_ptr[i] = GATE_UP ? We2 + (int64_t)min(n0 + b_row + 32 * i, N - 1) * K + b_c : nullptr;
    }
    f32x4 ga[2], gb[2], gb2[2];
    auto load_w = [&](const WT* p, f32x4 (&dst)[2], int k0, int i) {
        if constexpr (BF) {
            const u32x4 q = *reinterpret_cast<const u32x4*>(p + k0);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                dst[0][2 * c] = __uint_as_float(q[c] << 16);
                dst[0][2 * c + 1] = __uint_as_float(q[c] & 0xFFFF0000u);
                dst[1][2 * c] = __uint_as_float(q[2 + c] << 16);
                dst[1][2 * c + 1] = __uint_as_float(q[2 + c] & 0xFFFF0000u);
            }
        } else {
            dst[i] = *reinterpret_cast<const f32x4*>(p + k0);
        }
    };
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) ga[i] = *reinterpret_cast<const f32x4*>(a_ptr[i] + k0);
        if constexpr (BF) {
            load_w(b_ptr[0], gb, k0, 0);
            if constexpr (GATE_UP) load_w(b2_ptr[0], gb2, k0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                load_w(b_ptr[i], gb, k0, i);
                if constexpr (GATE_UP) load_w(b2_ptr[i], gb2, k0, i);
            }
        }
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&sA[stage][(a_row + 32 * i) * MG_STRIDE + a_c4 * 4]) = ga[i];
            // bf16: the thread's 8 values are consecutive in one row; f32: one float4 in each of two rows
            const int at = BF ? b_row * MG_STRIDE + b_c + 4 * i : (b_row + 32 * i) * MG_STRIDE + b_c;
            *reinterpret_cast<f32x4*>(&sB[stage][at]) = gb[i];
            if constexpr (GATE_UP) *reinterpret_cast<f32x4*>(&sB2[stage][at]) = gb2[i];
        }
    };

    f32x16 acc, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc2[r] = 0.0f;
    const int nk = K / MG_BK;
    const int fa = (wr * 32 + l31) * MG_STRIDE + half * 4, fb = (wc * 32 + l31) * MG_STRIDE + half * 4;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * MG_BK);
#pragma unroll
        for (int kk = 0; kk < MG_BK / 8; ++kk) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(&sA[cur][fa + kk * 8]);
            const f32x4 b = *reinterpret_cast<const f32x4*>(&sB[cur][fb + kk * 8]);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b[c], acc, 0, 0, 0);
            if constexpr (GATE_UP) {
                const f32x4 b2 = *reinterpret_cast<const f32x4*>(&sB2[cur][fb + kk * 8]);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], b2[c], acc2, 0, 0, 0);
            }
        }
        if (kt + 1 < nk) store(cur ^ 1);
        __syncthreads();
    }
    const int col = n0 + wc * 32 + l31;
    if (col < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = wr * 32 + acc_row(r, half);
            if (rr < cnt) out[(int64_t)s_slot[rr] * N + col] = GATE_UP ? silu(acc[r]) * acc2[r] : acc[r];
        }
    }
}

// Y[row] = R[row] + sum_j w[row, j] * y[row * k + j], j in order; float4 per thread.
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const float* __restrict__ weights, int rows, int k, int H,
                                                          const float* R, int64_t ldr, float* Y, int64_t ldy)
{
    const int h4 = H >> 2;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * h4) return;
    const int row = (int)(idx / h4), c = (int)(idx % h4) * 4;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < k; ++j) {
        const float w = weights[row * k + j];
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + ((int64_t)row * k + j) * H + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = fmaf(w, v[q], s[q]);
    }
    const f32x4 r = *reinterpret_cast<const f32x4*>(R + (int64_t)row * ldr + c);
    *reinterpret_cast<f32x4*>(Y + (int64_t)row * ldy + c) = r + s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool route_shape(int E, int k) { return E >= 2 && E <= MOE_MAX_EXPERTS && k >= 1 && k <= MOE_MAX_TOPK && k <= E; }

}  // namespace

hipError_t launch_moe_route(const float* logits, int64_t ldl, int rows, int E, int k, int norm_topk, int32_t* ids, float* weights,
                            hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!route_shape(E, k) || ldl < E) return hipErrorInvalidValue;
    hipLaunchKernelGGL(moe_route_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, logits, ldl, rows, E, k, norm_topk, ids, weights);
    return hipGetLastError();
}

hipError_t launch_moe_gate_up(const float* X, int64_t ldx, int rows, const float* gamma, float eps, const int32_t* ids, int k, int E,
                              const void* gate, const void* up, int bf16, int H, int Im, float* mid, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!route_shape(E, k) || rows > 8 || (H & 7) || H < 8 || H > 8192 || Im % 32 || Im < 32 || (ldx & 3) || ldx < H || !aligned16(X) ||
        !aligned16(gate) || !aligned16(up) || !aligned16(mid) || (gamma && !aligned16(gamma)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(Im / 16), (unsigned)(rows * k));
    const size_t lds = (size_t)H * sizeof(float);
    if (bf16)
        hipLaunchKernelGGL(moe_gate_up_kernel<uint16_t>, grid, dim3(256), lds, stream, X, ldx, gamma, eps, ids, k, E, static_cast<const uint16_t*>(gate),
                           static_cast<const uint16_t*>(up), H, Im, mid);
    else
        hipLaunchKernelGGL(moe_gate_up_kernel<float>, grid, dim3(256), lds, stream, X, ldx, gamma, eps, ids, k, E, static_cast<const float*>(gate),
                           static_cast<const float*>(up), H, Im, mid);
    return hipGetLastError();
}

hipError_t launch_moe_down_combine(const float* mid, int rows, const int32_t* ids, const float* weights, int k, int E, const void* down,
                                   int bf16, int H, int Im, const float* R, int64_t ldr, float* Y, int64_t ldy, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (!route_shape(E, k) || rows > 8 || (H & 7) || H < 8 || Im % 32 || Im < 32 || (int64_t)k * Im > 16384 || !R || ldr < H || ldy < H ||
        !aligned16(mid) || !aligned16(down))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(H / 8), (unsigned)rows);
    const size_t lds = (size_t)k * Im * sizeof(float);
    if (bf16)
        hipLaunchKernelGGL(moe_down_combine_kernel<uint16_t>, grid, dim3(256), lds, stream, mid, ids, weights, k, E, static_cast<const uint16_t*>(down),
                           H, Im, R, ldr, Y, ldy);
    else
        hipLaunchKernelGGL(moe_down_combine_kernel<float>, grid, dim3(256), lds, stream, mid, ids, weights, k, E, static_cast<const float*>(down), H, Im,
                           R, ldr, Y, ldy);
    return hipGetLastError();
}

int moe_max_tiles(int S, int E) { return S / MOE_TILE_ROWS + E; }  // sum over experts of ceil(count / 64) <= S / 64 + (experts with a remainder)

namespace {
size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }
}  // namespace

size_t moe_plan_ints(int S, int E) { return pad4((size_t)S) + pad4((size_t)E) + pad4((size_t)E + 1) + pad4(3 * (size_t)moe_max_tiles(S, E)) + 4; }

MoePlan moe_plan_at(int32_t* base, int S, int E)
{
    MoePlan p;
    p.sorted = base;
    p.counts = p.sorted + pad4((size_t)S);
    p.offsets = p.counts + pad4((size_t)E);
    p.tiles = p.offsets + pad4((size_t)E + 1);
    p.ntiles = p.tiles + pad4(3 * (size_t)moe_max_tiles(S, E));
    return p;
}

hipError_t launch_moe_group(const int32_t* ids, int S, int E, int32_t* plan, hipStream_t stream)
{
    if (S <= 0) return hipSuccess;
    if (E < 2 || E > MOE_MAX_EXPERTS) return hipErrorInvalidValue;
    const MoePlan p = moe_plan_at(plan, S, E);
    hipLaunchKernelGGL(moe_count_kernel, dim3((unsigned)E), dim3(64), 0, stream, ids, S, p.counts);
    hipLaunchKernelGGL(moe_place_kernel, dim3((unsigned)E), dim3(64), 0, stream, ids, S, E, p.counts, p.sorted, p.offsets, p.tiles, p.ntiles);
    return hipGetLastError();
}

hipError_t launch_moe_grouped_gemm(const float* A, int64_t lda, int a_div, const int32_t* plan, int S, int E, const void* W, const void* W2,
                                   int bf16, int N, int K, float* out, hipStream_t stream)
{
    if (S <= 0) return hipSuccess;
    if (E < 2 || E > MOE_MAX_EXPERTS || a_div < 1 || N < 1 || K < MG_BK || K % MG_BK || (lda & 3) || lda < K || !aligned16(A) || !aligned16(W) ||
        (W2 && !aligned16(W2)))
        return hipErrorInvalidValue;
    const MoePlan p = moe_plan_at(const_cast<int32_t*>(plan), S, E);
    const dim3 grid((unsigned)moe_max_tiles(S, E), (unsigned)((N + MG_BN - 1) / MG_BN));
#define KJ_MG(WT, GU)                                                                                                                      \
    hipLaunchKernelGGL((moe_grouped_gemm_kernel<WT, GU>), grid, dim3(256), 0, stream, A, lda, a_div, p.sorted, p.tiles, p.ntiles,          \
                       static_cast<const WT*>(W), static_cast<const WT*>(W2), N, K, out)
    if (bf16) {
        if (W2) KJ_MG(uint16_t, true);
        else KJ_MG(uint16_t, false);
    } else {
        if (W2) KJ_MG(float, true);
        else KJ_MG(float, false);
    }
#undef KJ_MG
    return hipGetLastError();
}

hipError_t launch_moe_combine(const float* y, const float* weights, int rows, int k, int H, const float* R, int64_t ldr, float* Y, int64_t ldy,
                              hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    if (k < 1 || k > MOE_MAX_TOPK || (H & 3) || !R || (ldr & 3) || (ldy & 3) || ldr < H || ldy < H || !aligned16(y) || !aligned16(R) || !aligned16(Y))
        return hipErrorInvalidValue;
    const int64_t total = (int64_t)rows * (H / 4);
    hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, y, weights, rows, k, H, R, ldr, Y, ldy);
    return hipGetLastError();
}

const char* moe_ffn_refusal(const MoeFfnArgs& a, bool grouped)
{
    if (a.E < 2 || a.E > MOE_MAX_EXPERTS) return "E must be 2 .. 256";
    if (a.k < 1 || a.k > MOE_MAX_TOPK || a.k > a.E) return "k must be 1 .. 8 and at most E";
    if (a.Im < 32 || a.Im % 32) return "Im must be a positive multiple of 32";
    if (a.H < 32 || a.H % 32 || a.H > 8192) return "hidden must be a multiple of 32, 32 .. 8192";
    if ((int64_t)a.k * a.Im > 16384) return "k * Im must be at most 16384";
    if (a.ldx < a.H || (a.ldx & 3) || a.ldr < a.H || (a.ldr & 3) || a.ldy < a.H || (a.ldy & 3)) return "ldx, ldr and ldy must cover hidden and be multiples of 4";
    if (!grouped && (a.rows < 0 || a.rows > 8)) return "the steps route takes at most 8 rows";
    if (grouped && a.gamma && a.ldx != a.H) return "the grouped route normalises contiguous rows (ldx == hidden)";
    return nullptr;
}

hipError_t launch_moe_ffn_steps(const MoeFfnArgs& a, hipStream_t stream)
{
    if (a.rows <= 0) return hipSuccess;
    if (moe_ffn_refusal(a, false)) return hipErrorInvalidValue;
    LlmGemvArgs g;
    g.X = a.X; g.ldx = a.ldx; g.rows = a.rows; g.gamma = a.gamma; g.eps = a.eps; g.W = a.router; g.bf16 = a.bf16; g.n_out = a.E; g.k = a.H;
    g.Y0 = a.logits; g.ldy0 = a.E;
    hipError_t e = launch_llm_gemv(g, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_route(a.logits, a.E, a.rows, a.E, a.k, a.norm_topk, a.ids, a.weights, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_gate_up(a.X, a.ldx, a.rows, a.gamma, a.eps, a.ids, a.k, a.E, a.gate, a.up, a.bf16, a.H, a.Im, a.mid, stream);
    if (e != hipSuccess) return e;
    return launch_moe_down_combine(a.mid, a.rows, a.ids, a.weights, a.k, a.E, a.down, a.bf16, a.H, a.Im, a.R, a.ldr, a.Y, a.ldy, stream);
}

hipError_t launch_moe_ffn_grouped(const MoeFfnArgs& a, hipStream_t stream)
{
    if (a.rows <= 0) return hipSuccess;
    if (moe_ffn_refusal(a, true)) return hipErrorInvalidValue;
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
    e = launch_moe_grouped_gemm(x, ldx, a.k, a.plan, S, a.E, a.gate, a.up, a.bf16, a.Im, a.H, a.mid, stream);
    if (e != hipSuccess) return e;
    e = launch_moe_grouped_gemm(a.mid, a.Im, 1, a.plan, S, a.E, a.down, nullptr, a.bf16, a.H, a.Im, a.y, stream);
    if (e != hipSuccess) return e;
    return launch_moe_combine(a.y, a.weights, a.rows, a.k, a.H, a.R, a.ldr, a.Y, a.ldy, stream);
}

}  // namespace kjarni
