// Compact lane KV caches (lane_kv_kernels.h): the encoding scatter, the prompt route's pack and the grouped-query ragged attention.
#include "lane_kv_kernels.h"

#include <math.h>

#include <algorithm>

#include "device_utils.h"
#include "fp8_decode.h"
#include "whisper_kernels.h"

namespace kjarni {

namespace {

constexpr int KV_MAX_CHUNK = 512;  // keys per split (launch_decode_attention's range rule)
constexpr float kF8Max = 448.0f;

// Two values as two e4m3 codes in bits [0, 16): scaled, clamped (no code is NaN), v_cvt_pk_fp8_f32 rounds to nearest even.
__device__ __forceinline__ uint32_t f8_pack2(float a, float b, float inv)
{
    const float x = fminf(fmaxf(a * inv, -kF8Max), kF8Max), y = fminf(fmaxf(b * inv, -kF8Max), kF8Max);
    if (inv == 0.0f) return 0u;  // (a head row of zeros stores codes 0, whatever the zeros' signs)
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, y, 0, false) & 0xffffu;
}

// ---- scatter ---------------------------------------------------------------------------------------------------------------------
// One workgroup per lane, its four waves stride over the lane's n_heads + 2 n_kv_heads heads (Q | K | V in the staging row); lane
// i < d/2 of the wave holds elements i and i + d/2 of the head -- the rotation's pair -- so the head norm's sum of squares and the
// FP8 amax are one wave reduction each.  The arithmetic up to the value that is stored is lane_rope_scatter_kernel's /
// head_norm_rope's (llm_kernels.hip), expression for expression.
template <int TYPE, bool NORM>
__global__ __launch_bounds__(256) void lane_scatter_kv_kernel(float* __restrict__ qkv, int64_t ld, int n_heads, int n_kv_heads, int head_dim,
                                                              const float* __restrict__ gamma_q, const float* __restrict__ gamma_k,
                                                              float eps, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                              uint8_t* __restrict__ Kc, uint8_t* __restrict__ Vc, float* __restrict__ Ks,
                                                              float* __restrict__ Vs, int64_t lane_rows, int capacity,
                                                              const int* __restrict__ pos, const int* __restrict__ live, int rotate)
{
    const int ln = blockIdx.x;
    if (!live[ln]) return;
    const int p = pos[ln];
    if (p < 0 || p >= capacity) return;
    const int half = head_dim >> 1, kv = n_kv_heads * head_dim;
    float* row = qkv + (int64_t)ln * ld;
    const int64_t r = (int64_t)ln * lane_rows + p;  // the lane's cache row, in rows of either plane
    const int lane = threadIdx.x & 63;
    const bool on = lane < half;
    for (int h = threadIdx.x >> 6; h < n_heads + 2 * n_kv_heads; h += 4) {  // (uniform over the wave)
        const bool is_q = h < n_heads, is_v = h >= n_heads + n_kv_heads;
        float* x = row + h * head_dim;
        const float x0 = on ? x[lane] : 0.0f, x1 = on ? x[lane + half] : 0.0f;
        float y0 = x0, y1 = x1;
        if (!is_v) {
            if (NORM) {
                float s = fmaf(x0, x0, 0.0f);
                s = fmaf(x1, x1, s);
                const float rms = sqrtf(wave_sum(s) / (float)head_dim + eps);
                const float* gamma = is_q ? gamma_q : gamma_k;
                const float g0 = on ? gamma[lane] : 0.0f, g1 = on ? gamma[lane + half] : 0.0f;
                y0 = (x0 / rms) * g0;
                y1 = (x1 / rms) * g1;
            }
            if (rotate) {
                const float c = on ? cos_t[(int64_t)p * half + lane] : 0.0f, sn = on ? sin_t[(int64_t)p * half + lane] : 0.0f;
                const float a = y0, b = y1;
                y0 = a * c - b * sn;
                y1 = a * sn + b * c;
            }
        }
        if (is_q) {
            if (on && (NORM || rotate)) {
                x[lane] = y0;
                x[lane + half] = y1;
            }
            continue;
        }
        const int kh = is_v ? h - n_heads - n_kv_heads : h - n_heads;
        const int64_t at = r * kv + kh * head_dim;  // the head's first element in the code plane
        uint8_t* codes = is_v ? Vc : Kc;
        if (TYPE == LANE_KV_BF16) {
            const uint32_t pk = sp_pack(y0, y1);
            uint16_t* d = reinterpret_cast<uint16_t*>(codes) + at;
            if (on) {
                d[lane] = (uint16_t)(pk & 0xffffu);
                d[lane + half] = (uint16_t)(pk >> 16);
            }
        } else {
            const float amax = wave_max(fmaxf(fabsf(y0), fabsf(y1)));  // (the lanes past d/2 hold zeros)
            const float inv = amax > 0.0f ? kF8Max / amax : 0.0f;
            const uint32_t pk = f8_pack2(y0, y1, inv);
            uint8_t* d = codes + at;
            if (on) {
                d[lane] = (uint8_t)(pk & 0xffu);
                d[lane + half] = (uint8_t)(pk >> 8);
            }
            if (lane == 0) (is_v ? Vs : Ks)[r * n_kv_heads + kh] = amax / kF8Max;
        }
    }
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// grid (x, 2 * layers): blockIdx.y picks the layer and K or V.  A 16-lane row of a wave takes one (cache row, head) at a time, lane
// j < d/8 of it eight consecutive floats (two 16-byte loads) -> eight codes (one 16-byte or 8-byte store); the FP8 amax is a DPP
// reduction over the row, the scale written by its lane 0.
template <int TYPE>
__global__ __launch_bounds__(256) void lane_kv_pack_kernel(const LaneKvPackEntry* __restrict__ table, int lane, int64_t lane_rows, int rows,
                                                           int n_kv_heads, int head_dim)
{
    const LaneKvPackEntry e = table[blockIdx.y >> 1];
    const bool v = (blockIdx.y & 1) != 0;
    const float* __restrict__ src = v ? e.src_v : e.src_k;
    uint8_t* __restrict__ dst = static_cast<uint8_t*>(v ? e.dst_v : e.dst_k);
    float* __restrict__ sc = v ? e.dst_v_scale : e.dst_k_scale;
    const int j = threadIdx.x & 15, kv = n_kv_heads * head_dim;
    const bool on = j < (head_dim >> 3);
    const int units = rows * n_kv_heads;
    for (int u = blockIdx.x * 16 + (threadIdx.x >> 4); u < units; u += gridDim.x * 16) {  // (uniform over the 16-lane row)
        const int rowi = u / n_kv_heads, kh = u - rowi * n_kv_heads;
        const float* s = src + (int64_t)rowi * kv + kh * head_dim + j * 8;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 a = on ? *reinterpret_cast<const f32x4*>(s) : zero, b = on ? *reinterpret_cast<const f32x4*>(s + 4) : zero;
        const int64_t r = (int64_t)lane * lane_rows + rowi;
        const int64_t at = r * kv + kh * head_dim + j * 8;
        if (TYPE == LANE_KV_BF16) {
            const u32x4 o = {sp_pack(a[0], a[1]), sp_pack(a[2], a[3]), sp_pack(b[0], b[1]), sp_pack(b[2], b[3])};
            if (on) *reinterpret_cast<u32x4*>(dst + at * 2) = o;
        } else {
            float m = fmaxf(fmaxf(fmaxf(fabsf(a[0]), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3]))),
                            fmaxf(fmaxf(fabsf(b[0]), fabsf(b[1])), fmaxf(fabsf(b[2]), fabsf(b[3]))));
            const float amax = row16_max_desc(m);
            const float inv = amax > 0.0f ? kF8Max / amax : 0.0f;
            const u32x2 o = {f8_pack2(a[0], a[1], inv) | (f8_pack2(a[2], a[3], inv) << 16), f8_pack2(b[0], b[1], inv) | (f8_pack2(b[2], b[3], inv) << 16)};
            if (on) *reinterpret_cast<u32x2*>(dst + at) = o;
            if (j == 0) sc[r * n_kv_heads + kh] = amax / kF8Max;
        }
    }
}

// ---- attention -------------------------------------------------------------------------------------------------------------------
// Sum over an aligned group of lpk (1, 2, 4, 8, 16) lanes, in every lane of it: the quad permutations are exact; once the quads are
// uniform row_half_mirror's lane 7 - i holds what lane i ^ 4 holds; row_ror:8 reads lane i ^ 8.  All lanes of the wave are active.
__device__ __forceinline__ float key_group_sum(float v, int lpk)
{
    if (lpk >= 2) v += dpp_mov<kDppQuadXor1>(v);
    if (lpk >= 4) v += dpp_mov<kDppQuadXor2>(v);
    if (lpk >= 8) v += dpp_mov<kDppRowHalfMirror>(v);
    if (lpk >= 16) v += dpp_mov<kDppRowRor + 8>(v);
    return v;
}
// Sum over the wave's lanes i with the same i % lpk, in every lane: rotations of the 16-lane row by lpk, 2 lpk, .. 8 (each adds the
// lanes one stride further round the row), then the rows by the permlane swaps.
__device__ __forceinline__ float key_column_sum(float v, int lpk)
{
    if (lpk <= 1) v += dpp_mov<kDppRowRor + 1>(v);
    if (lpk <= 2) v += dpp_mov<kDppRowRor + 2>(v);
    if (lpk <= 4) v += dpp_mov<kDppRowRor + 4>(v);
    if (lpk <= 8) v += dpp_mov<kDppRowRor + 8>(v);
    return sum_xor32(sum_xor16(v));
}

// The 16-byte piece as W floats: bf16 by a shift (8 values), FP8 by the packed converts (16 values, unscaled).
template <int TYPE>
__device__ __forceinline__ void widen(u32x4 p, float (&w)[TYPE == LANE_KV_BF16 ? 8 : 16])
{
    if constexpr (TYPE == LANE_KV_BF16) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            w[2 * d] = __uint_as_float(p[d] << 16);
            w[2 * d + 1] = __uint_as_float(p[d] & 0xffff0000u);
        }
    } else {
        decode16(p, w);
    }
}

// Workgroup (KV head x chunk of <= 8 of its query heads, split, lane); GT = the chunk's heads rounded up to a power of two (the
// heads past gcnt run with Q = 0 and are not written).  A key takes lpk = d / W lanes (W = 8 bf16 or 16 FP8 values per 16-byte
// piece), so 256 / lpk keys are in flight per trip.  The K pass holds the chunk's Q (staged through LDS) in GT x W registers and
// forms GT dots per key, reduced over the key's lanes by DPP; scores [GT][512] in LDS; max and sum per query head; the V pass walks
// the same rows once with GT x W accumulators (they take the registers Q leaves), reduced over the wave's keys by DPP / permlane
// swaps and over the four waves through LDS (the scores' buffer).  FP8: the row's scale is read once per key and multiplies the
// reduced dot (K) or the probability (V).  Slab layout and empty slabs: decode_attention_partial_kernel's.
template <int TYPE, int GT>
__global__ __launch_bounds__(256) void lane_attention_kv_kernel(const float* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ K0,
                                                                const uint8_t* __restrict__ V0, const float* __restrict__ KS0,
                                                                const float* __restrict__ VS0, int64_t lane_rows, int capacity,
                                                                int n_kv_heads, int group, int head_dim, float scale, int splits,
                                                                float* __restrict__ part, const int* __restrict__ lane_pos,
                                                                const int* __restrict__ lane_live)
{
    constexpr int W = TYPE == LANE_KV_BF16 ? 8 : 16;
    constexpr int ES = TYPE == LANE_KV_BF16 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) float buf[GT * KV_MAX_CHUNK];  // scores [GT][512], then accumulators [4][GT][head_dim]
    __shared__ __attribute__((aligned(16))) float qs[GT * 128];
    __shared__ float red[4 * GT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = (group + 7) >> 3;
    const int kvh = blockIdx.x / chunks, ck = blockIdx.x - kvh * chunks;
    const int gcnt = min(8, group - ck * 8), h0 = kvh * group + ck * 8, heads = n_kv_heads * group;
    const int sp = blockIdx.y, s = blockIdx.z;
    const int64_t hstride = (int64_t)splits * (head_dim + 4);  // from a head's slab to the next head's
    float* out0 = part + (((int64_t)s * heads + h0) * splits + sp) * (head_dim + 4);
    const int d4 = head_dim >> 2;
    const int n = lane_live[s] ? min(lane_pos[s] + 1, capacity) : 0;
    if (n <= 0) {
        for (int i = tid; i < gcnt * d4; i += 256) {
            const int j = i / d4, c = i - j * d4;
            *reinterpret_cast<f32x4*>(out0 + j * hstride + 4 + c * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (tid < gcnt) *reinterpret_cast<f32x4*>(out0 + tid * hstride) = f32x4{-INFINITY, 0.0f, 0.0f, 0.0f};
        return;
    }
    const int chunk = (n + splits - 1) / splits;
    const int t0 = sp * chunk, t1 = min(n, t0 + chunk), cnt = max(t1 - t0, 0), last = max(t1 - 1, t0);
    const int lpk = head_dim / W, groups = 256 / lpk;
    const int g = tid / lpk, l = tid - g * lpk;
    const int kv = n_kv_heads * head_dim;
    const int64_t row_bytes = (int64_t)kv * ES;
    const uint8_t* __restrict__ K = K0 + ((int64_t)s * lane_rows * kv + kvh * head_dim) * ES + l * 16;
    const uint8_t* __restrict__ V = V0 + ((int64_t)s * lane_rows * kv + kvh * head_dim) * ES + l * 16;
    const float* __restrict__ KS = TYPE == LANE_KV_BF16 ? nullptr : KS0 + (int64_t)s * lane_rows * n_kv_heads + kvh;
    const float* __restrict__ VS = TYPE == LANE_KV_BF16 ? nullptr : VS0 + (int64_t)s * lane_rows * n_kv_heads + kvh;

    for (int i = tid; i < GT * head_dim; i += 256) {
        const int j = i / head_dim;
        qs[i] = j < gcnt ? q[(int64_t)s * ldq + (int64_t)(h0 + j) * head_dim + (i - j * head_dim)] : 0.0f;
    }
    __syncthreads();

    float mx[GT], sum[GT];
#pragma unroll
    for (int j = 0; j < GT; ++j) {
        mx[j] = -INFINITY;
        sum[j] = 0.0f;
    }
    {  // (an empty range runs no trip: nothing is read)
        float qr[GT][W];
#pragma unroll
        for (int j = 0; j < GT; ++j) {
#pragma unroll
            for (int c = 0; c < W; c += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(qs + j * head_dim + l * W + c);
                qr[j][c] = t[0];
                qr[j][c + 1] = t[1];
                qr[j][c + 2] = t[2];
                qr[j][c + 3] = t[3];
            }
        }
        for (int tb = t0; tb < t1; tb += groups) {  // (uniform: the trip's keys past the range re-read the last row and are dropped)
            const int t = tb + g, tc = min(t, last);
            const u32x4 p = *reinterpret_cast<const u32x4*>(K + (int64_t)tc * row_bytes);
            float ks = 1.0f;
            if (TYPE != LANE_KV_BF16) ks = KS[(int64_t)tc * n_kv_heads];
            float kf[W];
            widen<TYPE>(p, kf);
#pragma unroll
            for (int j = 0; j < GT; ++j) {
                float dot = 0.0f;
#pragma unroll
                for (int c = 0; c < W; ++c) dot = fmaf(qr[j][c], kf[c], dot);
                dot = key_group_sum(dot, lpk);
                if (TYPE != LANE_KV_BF16) dot *= ks;
                const float v = dot * scale;
                if (t < t1) {
                    if (l == 0) buf[j * KV_MAX_CHUNK + (t - t0)] = v;
                    mx[j] = fmaxf(mx[j], v);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < GT; ++j) {
        const float m = wave_max(mx[j]);
        if (lane == 0) red[wave * GT + j] = m;
    }
    __syncthreads();  // (also: every score is in LDS)
#pragma unroll
    for (int j = 0; j < GT; ++j) mx[j] = fmaxf(fmaxf(red[j], red[GT + j]), fmaxf(red[2 * GT + j], red[3 * GT + j]));
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GT; ++j) {
        for (int i = tid; i < cnt; i += 256) {
            const float e = expf(buf[j * KV_MAX_CHUNK + i] - mx[j]);
            buf[j * KV_MAX_CHUNK + i] = e;
            sum[j] += e;
        }
        const float t = wave_sum(sum[j]);
        if (lane == 0) red[wave * GT + j] = t;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < GT; ++j) sum[j] = (red[j] + red[GT + j]) + (red[2 * GT + j] + red[3 * GT + j]);

    float acc[GT][W];
#pragma unroll
    for (int j = 0; j < GT; ++j) {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[j][c] = 0.0f;
    }
    for (int tb = t0; tb < t1; tb += groups) {
        const int t = tb + g, tc = min(t, last);
        const u32x4 p = *reinterpret_cast<const u32x4*>(V + (int64_t)tc * row_bytes);
        float vs = t < t1 ? 1.0f : 0.0f;
        if (TYPE != LANE_KV_BF16) vs *= VS[(int64_t)tc * n_kv_heads];
        float vf[W];
        widen<TYPE>(p, vf);
#pragma unroll
        for (int j = 0; j < GT; ++j) {
            const float pj = buf[j * KV_MAX_CHUNK + (tc - t0)] * vs;
#pragma unroll
            for (int c = 0; c < W; ++c) acc[j][c] = fmaf(pj, vf[c], acc[j][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < GT; ++j) {
#pragma unroll
        for (int c = 0; c < W; ++c) acc[j][c] = key_column_sum(acc[j][c], lpk);
    }
    __syncthreads();  // (the scores have been read: their buffer takes the waves' accumulators)
    if (lane < lpk) {
#pragma unroll
        for (int j = 0; j < GT; ++j) {
#pragma unroll
            for (int c = 0; c < W; c += 4)
                *reinterpret_cast<f32x4*>(buf + (wave * GT + j) * head_dim + lane * W + c) = f32x4{acc[j][c], acc[j][c + 1], acc[j][c + 2], acc[j][c + 3]};
        }
    }
    __syncthreads();
    const int wstride = GT * head_dim;
    for (int i = tid; i < gcnt * d4; i += 256) {
        const int j = i / d4, c = i - j * d4;
        const float* a = buf + j * head_dim + c * 4;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + wstride),
                    a2 = *reinterpret_cast<const f32x4*>(a + 2 * wstride), a3 = *reinterpret_cast<const f32x4*>(a + 3 * wstride);
        *reinterpret_cast<f32x4*>(out0 + j * hstride + 4 + c * 4) = (a0 + a1) + (a2 + a3);
    }
#pragma unroll
    for (int j = 0; j < GT; ++j)
        if (tid == j && j < gcnt) *reinterpret_cast<f32x4*>(out0 + j * hstride) = f32x4{cnt > 0 ? mx[j] : -INFINITY, cnt > 0 ? sum[j] : 0.0f, 0.0f, 0.0f};
}

bool compact(int type) { return type == LANE_KV_BF16 || type == LANE_KV_F8_E4M3; }

bool scatter_refuses(int type, int lanes, int n_heads, int n_kv_heads, int head_dim, int64_t lane_rows, int capacity, const LaneStateRef& state,
                     const void* kc, const void* vc, const float* ks, const float* vs)
{
    return !compact(type) || lanes > state.width || head_dim < 16 || head_dim > 128 || (head_dim & 15) || n_heads < 1 || n_kv_heads < 1 ||
           capacity < 0 || lane_rows < capacity || !kc || !vc || (type == LANE_KV_F8_E4M3 && (!ks || !vs));
}

}  // namespace

hipError_t launch_lane_rope_scatter_kv(int type, float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                       const float* cos_t, const float* sin_t, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                       int64_t lane_rows, int capacity, LaneStateRef state, int rotate, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (scatter_refuses(type, lanes, n_heads, n_kv_heads, head_dim, lane_rows, capacity, state, k_codes, v_codes, k_scale, v_scale))
        return hipErrorInvalidValue;
    auto kern = type == LANE_KV_BF16 ? lane_scatter_kv_kernel<LANE_KV_BF16, false> : lane_scatter_kv_kernel<LANE_KV_F8_E4M3, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)lanes), dim3(256), 0, stream, qkv, ld, n_heads, n_kv_heads, head_dim, nullptr, nullptr, 0.0f, cos_t,
                       sin_t, static_cast<uint8_t*>(k_codes), static_cast<uint8_t*>(v_codes), k_scale, v_scale, lane_rows, capacity, state.pos,
                       state.live, rotate ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_lane_qk_norm_rope_scatter_kv(int type, float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                               const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                               void* k_codes, void* v_codes, float* k_scale, float* v_scale, int64_t lane_rows, int capacity,
                                               LaneStateRef state, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (!gamma_q || !gamma_k || scatter_refuses(type, lanes, n_heads, n_kv_heads, head_dim, lane_rows, capacity, state, k_codes, v_codes, k_scale, v_scale))
        return hipErrorInvalidValue;
    auto kern = type == LANE_KV_BF16 ? lane_scatter_kv_kernel<LANE_KV_BF16, true> : lane_scatter_kv_kernel<LANE_KV_F8_E4M3, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)lanes), dim3(256), 0, stream, qkv, ld, n_heads, n_kv_heads, head_dim, gamma_q, gamma_k, eps, cos_t,
                       sin_t, static_cast<uint8_t*>(k_codes), static_cast<uint8_t*>(v_codes), k_scale, v_scale, lane_rows, capacity, state.pos,
                       state.live, 1);
    return hipGetLastError();
}

hipError_t launch_lane_kv_pack(int type, const LaneKvPackEntry* table, int layers, int lane, int64_t lane_rows, int rows, int n_kv_heads,
                               int head_dim, hipStream_t stream)
{
    if (layers <= 0 || rows <= 0) return hipSuccess;
    if (!compact(type) || !table || layers > 32767 || lane < 0 || rows > lane_rows || n_kv_heads < 1 || head_dim < 16 || head_dim > 128 ||
        (head_dim & 15))
        return hipErrorInvalidValue;
    const int64_t units = (int64_t)rows * n_kv_heads;
    if (units > (int64_t)1 << 30) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)std::min<int64_t>((units + 15) / 16, 256);
    auto kern = type == LANE_KV_BF16 ? lane_kv_pack_kernel<LANE_KV_BF16> : lane_kv_pack_kernel<LANE_KV_F8_E4M3>;
    hipLaunchKernelGGL(kern, dim3(blocks, (unsigned)(2 * layers)), dim3(256), 0, stream, table, lane, lane_rows, rows, n_kv_heads, head_dim);
    return hipGetLastError();
}

bool lane_attention_kv_accepts(int type, int lanes, int capacity, int heads, int n_kv_heads, int head_dim, int splits)
{
    if (!compact(type) || lanes < 1 || lanes > kMaxWideLanes || capacity < 1 || splits < 1) return false;
    if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) return false;
    if (n_kv_heads < 1 || heads < n_kv_heads || heads % n_kv_heads) return false;
    return (capacity + splits - 1) / splits <= KV_MAX_CHUNK;
}

hipError_t launch_lane_attention_kv(int type, const float* q, int64_t ldq, int lanes, const void* k_codes, const void* v_codes,
                                    const float* k_scale, const float* v_scale, int64_t lane_rows, int capacity, int heads, int n_kv_heads,
                                    int head_dim, int splits, float* scratch, float* ctx, int64_t ldc, const int* lane_pos,
                                    const int* lane_live, hipStream_t stream)
{
    if (lanes <= 0) return hipSuccess;
    if (!lane_attention_kv_accepts(type, lanes, capacity, heads, n_kv_heads, head_dim, splits) || !q || !k_codes || !v_codes || !scratch ||
        !lane_pos || !lane_live || lane_rows < capacity || (type == LANE_KV_F8_E4M3 && (!k_scale || !v_scale)))
        return hipErrorInvalidValue;
    const int group = heads / n_kv_heads, chunks = (group + 7) / 8;
    const dim3 grid((unsigned)(n_kv_heads * chunks), (unsigned)splits, (unsigned)lanes);
    const float scale = 1.0f / sqrtf((float)head_dim);
    const uint8_t* K = static_cast<const uint8_t*>(k_codes);
    const uint8_t* V = static_cast<const uint8_t*>(v_codes);
#define KJ_LKV(TYPE, GT)                                                                                                                 \
    hipLaunchKernelGGL((lane_attention_kv_kernel<TYPE, GT>), grid, dim3(256), 0, stream, q, ldq, K, V, k_scale, v_scale, lane_rows, capacity, \
                       n_kv_heads, group, head_dim, scale, splits, scratch, lane_pos, lane_live)
#define KJ_LKV_G(TYPE)                                                                                                                   \
    do {                                                                                                                                 \
        if (group == 1) KJ_LKV(TYPE, 1);                                                                                                 \
        else if (group == 2) KJ_LKV(TYPE, 2);                                                                                            \
        else if (group <= 4) KJ_LKV(TYPE, 4);                                                                                            \
        else KJ_LKV(TYPE, 8);                                                                                                            \
    } while (0)
    if (type == LANE_KV_BF16) KJ_LKV_G(LANE_KV_BF16);
    else KJ_LKV_G(LANE_KV_F8_E4M3);
#undef KJ_LKV_G
#undef KJ_LKV
    if (ctx) return launch_decode_attention_combine(scratch, lanes, heads, splits, head_dim, ctx, ldc, stream);
    return hipGetLastError();
}

}  // namespace kjarni
