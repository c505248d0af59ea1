// Compact single-sequence KV cache (seq_kv_kernels.h): the row-indexed encoding scatter and the rows attention over the codes.
#include "seq_kv_kernels.h"

#include <math.h>

#include <algorithm>

#include "device_utils.h"
#include "fp8_decode.h"
#include "whisper_kernels.h"

namespace kjarni {

namespace {

constexpr float kF8Max = 448.0f;

// lane_kv_kernels.hip's pair encoder: scaled, clamped (no code is NaN), v_cvt_pk_fp8_f32 rounds to nearest even.
__device__ __forceinline__ uint32_t f8_pack2(float a, float b, float inv)
{
    const float x = fminf(fmaxf(a * inv, -kF8Max), kF8Max), y = fminf(fmaxf(b * inv, -kF8Max), kF8Max);
    if (inv == 0.0f) return 0u;  // (a head row of zeros stores codes 0, whatever the zeros' signs)
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, y, 0, false) & 0xffffu;
}

// ---- scatter ---------------------------------------------------------------------------------------------------------------------
// lane_scatter_kv_kernel with "lane" read as "row of the block": one workgroup per row, its four waves stride over the row's
// n_heads + 2 n_kv_heads heads; lane i < d/2 of the wave holds elements i and i + d/2 of the head.
template <int TYPE, bool NORM>
__global__ __launch_bounds__(256) void seq_kv_scatter_kernel(float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                             const float* __restrict__ v, int64_t ldv, int n_heads, int n_kv_heads,
                                                             int head_dim, const float* __restrict__ gamma_q,
                                                             const float* __restrict__ gamma_k, float eps, const float* __restrict__ cos_t,
                                                             const float* __restrict__ sin_t, uint8_t* __restrict__ Kc,
                                                             uint8_t* __restrict__ Vc, float* __restrict__ Ks, float* __restrict__ Vs, int base,
                                                             const int* __restrict__ base_ptr, int capacity, int rotate)
{
    const int r = blockIdx.x;
    const int p = (base_ptr ? *base_ptr : base) + r;
    if (p < 0 || p >= capacity) return;
    const int half = head_dim >> 1, kv = n_kv_heads * head_dim;
    const int lane = threadIdx.x & 63;
    const bool on = lane < half;
    for (int h = threadIdx.x >> 6; h < n_heads + 2 * n_kv_heads; h += 4) {  // (uniform over the wave)
        const bool is_q = h < n_heads, is_v = h >= n_heads + n_kv_heads;
        const int kh = is_v ? h - n_heads - n_kv_heads : h - n_heads;
        const float* x = is_q ? q + (int64_t)r * ldq + h * head_dim : is_v ? v + (int64_t)r * ldv + kh * head_dim : k + (int64_t)r * ldk + kh * head_dim;
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
                float* xq = q + (int64_t)r * ldq + h * head_dim;
                xq[lane] = y0;
                xq[lane + half] = y1;
            }
            continue;
        }
        const int64_t at = (int64_t)p * kv + kh * head_dim;  // the head's first element in the code plane
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
            if (lane == 0) (is_v ? Vs : Ks)[(int64_t)p * n_kv_heads + kh] = amax / kF8Max;
        }
    }
}

// ---- attention -------------------------------------------------------------------------------------------------------------------
// One wave per workgroup.  M tile: 32 (query row, group head) pairs of ONE KV head -- pair p is row r0 + p / gt, head h0 + p % gt,
// gt = the chunk's <= 8 heads rounded up to a power of two (pairs past the block's rows or the chunk's heads run with Q = 0 and are
// not written).  Both products are formed TRANSPOSED, so that a pair is a COLUMN of the accumulators (lane & 31) and the softmax
// state -- max, sum, the rescale factor -- is one register per lane, with one cross-lane step (lane ^ 32) per key tile:
//   S^T [32 keys x 32 pairs] = K Q^T   A = the K codes: lane (key = lane & 31, half = lane >> 5) loads the 8 consecutive elements
//                                      16 ks + 8 half .. of its key's head row straight from HBM (16 bytes bf16, 8 bytes FP8 widened
//                                      exactly by v_cvt_scalef32_pk_bf16_fp8); B = Q (pair = lane & 31), scaled by 1 / sqrt(d), split
//                                      once into three exact bf16 planes and held in registers for the whole key loop.
//   O^T [d x 32 pairs] += V^T P^T      B = P as it leaves the softmax: register 8 j + e of the S^T accumulator is element e of
//                                      k-step j (the keys of a k-step are then 8 j' + 4 half + (0..3) of two j': a permutation
//                                      the A side follows); P (times the FP8 V scale of its key) split into three planes.
//                                      A = V^T: the V pieces are loaded like K's, widened, and transposed through LDS into
//                                      Vt[dim][slot(key)], 80 bytes per dim, read back with one 16-byte load per fragment.
// FP8: the K scale of a key multiplies its score row in f32 after the MFMAs; the tile's 32 K and 32 V scales are loaded by lanes
// 0..31 and handed to the accumulator layout through LDS.  Keys past the slab re-read its last row and are masked; the causal and
// slab-end masks run only in tiles that reach past min(slab end, the block's first row's last key).  Slab layout and empty slabs:
// decode_attention_partial_kernel's.
constexpr int VT_STRIDE = 40;  // bf16 per dim row of Vt: 32 key slots + 8 of padding (rows stay 16-byte aligned)

__device__ __forceinline__ int vt_slot(int key)  // where key (0..31) of the tile sits in the k order of P's fragments
{
    const int q = key >> 3;
    return (q >> 1) * 16 + ((key >> 2) & 1) * 8 + (q & 1) * 4 + (key & 3);
}

template <int TYPE>
__device__ __forceinline__ u32x4 load_piece(const uint8_t* p)  // 8 codes as 8 bf16
{
    if constexpr (TYPE == LANE_KV_BF16) return *reinterpret_cast<const u32x4*>(p);
    else return fp8x8_to_bf16x8(*reinterpret_cast<const u32x2*>(p));
}

template <int TYPE, int D>
__global__ __launch_bounds__(64) void seq_attention_kv_kernel(const float* __restrict__ q, int64_t ldq, const uint8_t* __restrict__ K0,
                                                              const uint8_t* __restrict__ V0, const float* __restrict__ KS0,
                                                              const float* __restrict__ VS0, int base, const int* __restrict__ base_ptr,
                                                              int rows, int capacity, int n_kv_heads, int group, int gt, float qscale,
                                                              int splits, float* __restrict__ part)
{
    constexpr int ES = TYPE == LANE_KV_BF16 ? 2 : 1;
    constexpr int KS = D / 16;          // k-steps of S^T, and 8-element pieces per half of a key row
    constexpr int DT = (D + 31) / 32;   // 32-dim tiles of O^T
    __shared__ __attribute__((aligned(16))) uint16_t vt[DT * 32 * VT_STRIDE];
    __shared__ __attribute__((aligned(16))) float sc[2][32];
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int rb = 32 / gt, rbs = (rows + rb - 1) / rb, chunks = (group + 7) >> 3;
    const int rbi = blockIdx.x % rbs, t = blockIdx.x / rbs;
    const int ck = t % chunks, kvh = t / chunks;
    const int gcnt = min(8, group - ck * 8), h0 = kvh * group + ck * 8, heads = n_kv_heads * group;
    const int r0 = rbi * rb, sp = blockIdx.y;
    const int prow = r0 + l31 / gt, pj = l31 % gt;
    const bool pair_on = prow < rows && pj < gcnt;
    const int B0 = base_ptr ? *base_ptr : base;
    const int nk = min(B0 + min(r0 + rb, rows), capacity);  // the keys any row of the block sees
    const int chunk = (((nk + splits - 1) / splits) + 31) & ~31;
    const int t0 = sp * chunk, t1 = min(nk, t0 + chunk);
    const int kv = n_kv_heads * D;

    if (D < 32) {  // (the dims past d of the one O^T tile multiply zeros)
        for (int i = lane; i < 16 * VT_STRIDE; i += 64) vt[16 * VT_STRIDE + i] = 0;
    }

    // Q: this lane's pair, elements 16 ks + 8 half .. + 8, scaled and split once
    bf16x8 qb[KS][3];
    {
        const float* qrow = q + (int64_t)(pair_on ? prow : 0) * ldq + (int64_t)(h0 + (pair_on ? pj : 0)) * D + 8 * half;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
            if (pair_on) {
                a = *reinterpret_cast<const f32x4*>(qrow + ks * 16);
                b = *reinterpret_cast<const f32x4*>(qrow + ks * 16 + 4);
            }
            u32x2 a1, a2, a3, b1, b2, b3;
            sp_split(a * qscale, a1, a2, a3);
            sp_split(b * qscale, b1, b2, b3);
            qb[ks][0] = __builtin_bit_cast(bf16x8, u32x4{a1[0], a1[1], b1[0], b1[1]});
            qb[ks][1] = __builtin_bit_cast(bf16x8, u32x4{a2[0], a2[1], b2[0], b2[1]});
            qb[ks][2] = __builtin_bit_cast(bf16x8, u32x4{a3[0], a3[1], b3[0], b3[1]});
        }
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
    float mx = -INFINITY, sum = 0.0f;
    const int slot = vt_slot(l31);
    const int edge = min(t1, B0 + r0 + 1);  // tiles that end at or before it need no mask

    for (int kt = t0; kt < t1; kt += 32) {
        const int kc = min(kt + l31, t1 - 1);  // (keys past the slab re-read its last row and are masked)
        const int64_t at = ((int64_t)kc * kv + kvh * D + 8 * half) * ES;
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 a = __builtin_bit_cast(bf16x8, load_piece<TYPE>(K0 + at + ks * 16 * ES));
#pragma unroll
            for (int p = 2; p >= 0; --p) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qb[ks][p], s, 0, 0, 0);  // the smallest piece first
        }
        u32x4 vp[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) vp[ks] = load_piece<TYPE>(V0 + at + ks * 16 * ES);
        if (TYPE != LANE_KV_BF16) {
            if (half == 0) {
                sc[0][l31] = KS0[(int64_t)kc * n_kv_heads + kvh];
                sc[1][l31] = VS0[(int64_t)kc * n_kv_heads + kvh];
            }
        }
        // V^T into LDS: element e of piece ks is dim 16 ks + 8 half + e of key l31
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                vt[(ks * 16 + 8 * half + e) * VT_STRIDE + slot] = (uint16_t)(e & 1 ? vp[ks][e >> 1] >> 16 : vp[ks][e >> 1] & 0xffffu);
        __syncthreads();
        if (TYPE != LANE_KV_BF16) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 k4 = *reinterpret_cast<const f32x4*>(&sc[0][8 * g + 4 * half]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[4 * g + e] *= k4[e];
            }
        }
        if (kt + 32 > edge) {  // (uniform) the slab's end and the causal edge: key <= the row's position
            const int lim = min(t1 - 1, B0 + prow);
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (kt + acc_row(i, half) > lim) s[i] = -INFINITY;
        }
        float mt = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mt = fmaxf(mt, s[i]);
        mt = max_xor32(mt);
        const float mn = fmaxf(mx, mt), mu = mn == -INFINITY ? 0.0f : mn;  // (a pair with no key yet keeps max -inf, sum 0)
        const float alpha = expf(mx - mu);
        mx = mn;
        float ps = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            s[i] = expf(s[i] - mu);
            ps += s[i];
        }
        sum = sum * alpha + ps;
        if (TYPE != LANE_KV_BF16) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(&sc[1][8 * g + 4 * half]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[4 * g + e] *= v4[e];
            }
        }
        bf16x8 pb[2][3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32x2 a1, a2, a3, b1, b2, b3;
            sp_split(f32x4{s[8 * j], s[8 * j + 1], s[8 * j + 2], s[8 * j + 3]}, a1, a2, a3);
            sp_split(f32x4{s[8 * j + 4], s[8 * j + 5], s[8 * j + 6], s[8 * j + 7]}, b1, b2, b3);
            pb[j][0] = __builtin_bit_cast(bf16x8, u32x4{a1[0], a1[1], b1[0], b1[1]});
            pb[j][1] = __builtin_bit_cast(bf16x8, u32x4{a2[0], a2[1], b2[0], b2[1]});
            pb[j][2] = __builtin_bit_cast(bf16x8, u32x4{a3[0], a3[1], b3[0], b3[1]});
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(&vt[(dt * 32 + l31) * VT_STRIDE + j * 16 + half * 8]);
#pragma unroll
                for (int p = 2; p >= 0; --p) o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pb[j][p], o[dt], 0, 0, 0);
            }
        }
        __syncthreads();  // (Vt and the scales have been read: the next tile may overwrite them)
    }

    sum = sum_xor32(sum);  // the two halves hold the sums of their own keys, rescaled alike
    if (!pair_on) return;
    float* out = part + (((int64_t)prow * heads + h0 + pj) * splits + sp) * (D + 4);
    if (half == 0) *reinterpret_cast<f32x4*>(out) = f32x4{mx, sum, 0.0f, 0.0f};
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int dim = dt * 32 + 8 * g + 4 * half;
            if (dim < D) *reinterpret_cast<f32x4*>(out + 4 + dim) = f32x4{o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]};
        }
}

bool compact(int type) { return type == LANE_KV_BF16 || type == LANE_KV_F8_E4M3; }

}  // namespace

hipError_t launch_seq_kv_scatter(int type, float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, int rows,
                                 int n_heads, int n_kv_heads, int head_dim, const float* gamma_q, const float* gamma_k, float eps,
                                 const float* cos_t, const float* sin_t, void* k_codes, void* v_codes, float* k_scale, float* v_scale,
                                 int base, const int* base_ptr, int capacity, int rotate, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    const bool norm = gamma_q || gamma_k;
    if (!compact(type) || !q || !k || !v || head_dim < 16 || head_dim > 128 || (head_dim & 15) || n_heads < 1 || n_kv_heads < 1 ||
        capacity < 0 || (!base_ptr && (base < 0 || (int64_t)base + rows > capacity)) || !k_codes || !v_codes ||
        (type == LANE_KV_F8_E4M3 && (!k_scale || !v_scale)) || (norm && (!gamma_q || !gamma_k)) || ((norm || rotate) && (!cos_t || !sin_t)))
        return hipErrorInvalidValue;
#define KJ_SKS(TYPE, NORM)                                                                                                              \
    hipLaunchKernelGGL((seq_kv_scatter_kernel<TYPE, NORM>), dim3((unsigned)rows), dim3(256), 0, stream, q, ldq, k, ldk, v, ldv, n_heads,   \
                       n_kv_heads, head_dim, gamma_q, gamma_k, eps, cos_t, sin_t, static_cast<uint8_t*>(k_codes),                       \
                       static_cast<uint8_t*>(v_codes), k_scale, v_scale, base, base_ptr, capacity, (norm || rotate) ? 1 : 0)
    if (type == LANE_KV_BF16) {
        if (norm) KJ_SKS(LANE_KV_BF16, true);
        else KJ_SKS(LANE_KV_BF16, false);
    } else {
        if (norm) KJ_SKS(LANE_KV_F8_E4M3, true);
        else KJ_SKS(LANE_KV_F8_E4M3, false);
    }
#undef KJ_SKS
    return hipGetLastError();
}

bool seq_attention_kv_accepts(int type, int rows, int base, int capacity, int heads, int n_kv_heads, int head_dim, int splits)
{
    if (!compact(type) || rows < 1 || base < 0 || capacity < 1 || splits < 1 || splits > 65535) return false;
    if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) return false;
    if (n_kv_heads < 1 || heads < n_kv_heads || heads % n_kv_heads) return false;
    return (int64_t)base + rows <= capacity;
}

hipError_t launch_seq_attention_kv(int type, const float* q, int64_t ldq, int rows, const void* k_codes, const void* v_codes,
                                   const float* k_scale, const float* v_scale, int base, const int* base_ptr, int capacity, int heads,
                                   int n_kv_heads, int head_dim, int splits, float* scratch, float* ctx, int64_t ldc, hipStream_t stream)
{
    if (rows <= 0) return hipSuccess;
    // (a device-held base is the caller's to keep below capacity - rows; the kernel clamps its key range to the capacity)
    if (!seq_attention_kv_accepts(type, rows, base_ptr ? 0 : base, capacity, heads, n_kv_heads, head_dim, splits) || !q || !k_codes ||
        !v_codes || !scratch || (ldq & 3) || (reinterpret_cast<uintptr_t>(q) & 15) || (type == LANE_KV_F8_E4M3 && (!k_scale || !v_scale)))
        return hipErrorInvalidValue;
    const int group = heads / n_kv_heads, chunks = (group + 7) / 8;
    const int top = std::min(group, 8);
    const int gt = top <= 1 ? 1 : top <= 2 ? 2 : top <= 4 ? 4 : 8;
    const int rb = 32 / gt;
    const int64_t blocks = (int64_t)n_kv_heads * chunks * ((rows + rb - 1) / rb);
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)splits);
    const float qscale = 1.0f / sqrtf((float)head_dim);
    const uint8_t* K = static_cast<const uint8_t*>(k_codes);
    const uint8_t* V = static_cast<const uint8_t*>(v_codes);
#define KJ_SKV(TYPE, D)                                                                                                                  \
    hipLaunchKernelGGL((seq_attention_kv_kernel<TYPE, D>), grid, dim3(64), 0, stream, q, ldq, K, V, k_scale, v_scale, base, base_ptr, rows, \
                       capacity, n_kv_heads, group, gt, qscale, splits, scratch)
#define KJ_SKV_D(TYPE)                                                                                                                   \
    do {                                                                                                                                 \
        if (head_dim == 16) KJ_SKV(TYPE, 16);                                                                                            \
        else if (head_dim == 32) KJ_SKV(TYPE, 32);                                                                                       \
        else if (head_dim == 64) KJ_SKV(TYPE, 64);                                                                                       \
        else KJ_SKV(TYPE, 128);                                                                                                          \
    } while (0)
    if (type == LANE_KV_BF16) KJ_SKV_D(LANE_KV_BF16);
    else KJ_SKV_D(LANE_KV_F8_E4M3);
#undef KJ_SKV_D
#undef KJ_SKV
    if (ctx) return launch_decode_attention_combine(scratch, rows, heads, splits, head_dim, ctx, ldc, stream);
    return hipGetLastError();
}

}  // namespace kjarni
