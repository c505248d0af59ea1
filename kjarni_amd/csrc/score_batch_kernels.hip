// Kernels of batched scoring (LlmModel::score_batch): attention of a remainder over its shared prefix and its own rows, and the
// gather + final norm of the rows whose successor is scored.
//
//   attention   cpu/decoder/decoder_attention.rs:99-160, utils/masks.rs:103-113 (per sequence)
//   RMSNorm     cpu/normalization/rms_norm.rs:19-27
//   LayerNorm   cpu/normalization/layer_norm.rs:96-131
#include "score_batch_kernels.h"

#include "device_utils.h"
#include "dynamic_lds.h"

namespace kjarni {

namespace {

// packed_attention_kernel (decoder_embed_kernels.hip) on one query block of a remainder, over the virtual sequence "prefix rows,
// then the remainder's rows": 32 queries x 64-key tiles from virtual key 0, 8 threads per query, running (max, sum, output) per
// query.  Virtual key v is row prefix_first + v below prefix_len, else row first + v - prefix_len; the clamp keeps every load
// inside those two row ranges.
constexpr int PP_Q = 32, PP_K = 64;

template <int DPT>
__global__ __launch_bounds__(256) void packed_prefix_attention_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ K,
                                                                      int64_t ldk, const float* __restrict__ V, int64_t ldv,
                                                                      const PrefixBlock* __restrict__ blocks, int kv_group, float scale,
                                                                      float* __restrict__ ctx, int64_t ldc)
{
    constexpr int D = 8 * DPT, LD = D + 4;
    extern __shared__ __attribute__((aligned(16))) float pp_smem[];
    float* sQ = pp_smem;               // [PP_Q][LD]
    float* sK = sQ + PP_Q * LD;        // [PP_K][LD]
    float* sV = sK + PP_K * LD;        // [PP_K][LD]
    float* sP = sV + PP_K * LD;        // [PP_Q][PP_K + 4]
    const PrefixBlock pb = blocks[blockIdx.x];
    const int rows = pb.len, q0 = pb.q0, plen = pb.prefix_len;
    const int own_shift = pb.first - plen;  // virtual key v >= plen is row v + own_shift
    q += (int64_t)pb.first * ldq;
    ctx += (int64_t)pb.first * ldc;
    const int tid = threadIdx.x, qi = tid >> 3, kg = tid & 7;
    const int h = blockIdx.y, hk = h / kv_group;
    const int q_row = q0 + qi;
    const bool valid = q_row < rows;
    const int limit = plen + q_row;                           // last visible virtual key of this query
    const int last_key = plen + min(rows, q0 + PP_Q) - 1;     // last virtual key any query of the block sees
    for (int i = tid; i < PP_Q * (D / 4); i += 256) {
        const int r = i / (D / 4), c4 = i - r * (D / 4);
        const int row = min(q0 + r, rows - 1);
        *reinterpret_cast<f32x4*>(sQ + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(q + (int64_t)row * ldq + h * D + c4 * 4);
    }
    float m_run = -INFINITY, l_run = 0.0f;
    float o[DPT];
#pragma unroll
    for (int c = 0; c < DPT; ++c) o[c] = 0.0f;
    for (int k0 = 0; k0 <= last_key; k0 += PP_K) {
        __syncthreads();  // previous tile fully consumed (and sQ written, first trip)
        for (int i = tid; i < PP_K * (D / 4); i += 256) {
            const int r = i / (D / 4), c4 = i - r * (D / 4);
            const int key = min(k0 + r, last_key);
            const int64_t row = key < plen ? pb.prefix_first + key : key + own_shift;
            *reinterpret_cast<f32x4*>(sK + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(K + row * ldk + hk * D + c4 * 4);
            *reinterpret_cast<f32x4*>(sV + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(V + row * ldv + hk * D + c4 * 4);
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
            sP[qi * (PP_K + 4) + kg + 8 * j] = p;
        }
        psum = group8_sum_asc(psum);
        const float alpha = (m_new == -INFINITY || m_run == -INFINITY) ? (m_run == -INFINITY ? 0.0f : 1.0f) : expf(m_run - m_new);
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int c = 0; c < DPT; ++c) o[c] *= alpha;
        m_run = m_new;
        __syncthreads();  // the tile's probabilities are in LDS
        const int jn = valid ? min(PP_K, limit - k0 + 1) : 0;  // the tile's keys this query sees
        for (int j = 0; j < jn; ++j) {
            const float p = sP[qi * (PP_K + 4) + j];
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

// One workgroup per output row: row src[j] of x through the final RMSNorm, the statistic summed as rmsnorm_kernel sums it
// (lane-strided fmaf chains of one wave, then the wave-wide butterfly), as last_token_pool_kernel does without its L2 step.
__global__ __launch_bounds__(256) void score_gather_norm_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ src,
                                                                int hidden, const float* __restrict__ gamma, float eps,
                                                                float* __restrict__ out, int64_t ldo)
{
    __shared__ float red;
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = x + (int64_t)src[j] * ldx;
    if (wave == 0) {
        float s = 0.0f;
        for (int i = lane; i < hidden; i += 64) s = fmaf(row[i], row[i], s);
        s = wave_sum(s);
        if (lane == 0) red = s;
    }
    __syncthreads();
    const float rms = sqrtf(red / (float)hidden + eps);
    for (int i = tid; i < hidden; i += 256) out[(int64_t)j * ldo + i] = (row[i] / rms) * gamma[i];
}

// The LayerNorm form (GPT-2's ln_f): one wave per output row with layernorm_kernel's arithmetic (rowops.hip) -- V4: the row held
// as float4 registers, pairwise partial sums; else layernorm_generic_kernel's three passes.
constexpr int GN_V4_PER_LANE = 4;  // (MAX_V4_PER_LANE of rowops.hip: hidden <= 1024 on the float4 path)

template <bool V4>
__global__ __launch_bounds__(64) void score_gather_layernorm_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ src,
                                                                    int hidden, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps, float* __restrict__ out,
                                                                    int64_t ldo)
{
    const int j = blockIdx.x, lane = threadIdx.x;
    const float* irow = x + (int64_t)src[j] * ldx;
    float* orow = out + (int64_t)j * ldo;
    if constexpr (V4) {
        const int nv4 = hidden >> 2;
        f32x4 xr[GN_V4_PER_LANE];
#pragma unroll
        for (int i = 0; i < GN_V4_PER_LANE; ++i) {
            const int c4 = lane + i * 64;
            xr[i] = (c4 < nv4) ? *reinterpret_cast<const f32x4*>(irow + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < GN_V4_PER_LANE; ++i)
            if (lane + i * 64 < nv4) s += (xr[i][0] + xr[i][1]) + (xr[i][2] + xr[i][3]);
        const float mean = wave_sum(s) / (float)hidden;
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < GN_V4_PER_LANE; ++i)
            if (lane + i * 64 < nv4) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = xr[i][c] - mean;
                    v = fmaf(d, d, v);
                }
            }
        const float var = wave_sum(v) / (float)hidden;
        const float inv_std = 1.0f / sqrtf(var + eps);
#pragma unroll
        for (int i = 0; i < GN_V4_PER_LANE; ++i) {
            const int c4 = lane + i * 64;
            if (c4 < nv4) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c4 * 4);
                const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c4 * 4);
                f32x4 o;
#pragma unroll
                for (int c = 0; c < 4; ++c) o[c] = (xr[i][c] - mean) * inv_std * g[c] + b[c];
                *reinterpret_cast<f32x4*>(orow + c4 * 4) = o;
            }
        }
    } else {
        float s = 0.f;
        for (int i = lane; i < hidden; i += 64) s += irow[i];
        const float mean = wave_sum(s) / (float)hidden;
        float v = 0.f;
        for (int i = lane; i < hidden; i += 64) {
            const float d = irow[i] - mean;
            v = fmaf(d, d, v);
        }
        const float inv_std = 1.0f / sqrtf(wave_sum(v) / (float)hidden + eps);
        for (int i = lane; i < hidden; i += 64) {
            const float xv = irow[i];
            orow[i] = (xv - mean) * inv_std * gamma[i] + beta[i];
        }
    }
}

}  // namespace

hipError_t launch_packed_prefix_attention(const float* q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                                          const PrefixBlock* blocks, int n_blocks, int heads, int head_dim, int kv_group, float* ctx,
                                          int64_t ldc, hipStream_t stream)
{
    if (n_blocks <= 0) return hipSuccess;
    if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
    if (heads < 1 || ((ldq | ldk | ldv | ldc) & 3) != 0 ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(ctx)) & 15) != 0)
        return hipErrorInvalidValue;
    const int g = kv_group < 1 ? 1 : kv_group;
    const float scale = 1.0f / sqrtf((float)head_dim);
    const dim3 grid((unsigned)n_blocks, (unsigned)heads);
    const int LD = head_dim + 4;
    const size_t lds = ((size_t)(PP_Q + 2 * PP_K) * LD + (size_t)PP_Q * (PP_K + 4)) * sizeof(float);
#define KJ_PP(DPT)                                                                                                       \
    do {                                                                                                                 \
        auto kern = packed_prefix_attention_kernel<DPT>;                                                                 \
        if (lds > 48 * 1024) {                                                                                           \
            const hipError_t e = allow_dynamic_lds(kern, lds);                                                           \
            if (e != hipSuccess) return e;                                                                               \
        }                                                                                                                \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, q, ldq, K, ldk, V, ldv, blocks, g, scale, ctx, ldc);      \
    } while (0)
    switch (head_dim) {
    case 16: KJ_PP(2); break;
    case 32: KJ_PP(4); break;
    case 64: KJ_PP(8); break;
    default: KJ_PP(16); break;
    }
#undef KJ_PP
    return hipGetLastError();
}

hipError_t launch_score_gather_norm(const float* x, int64_t ldx, const int32_t* src, int n, int hidden, const float* gamma, const float* beta,
                                    float eps, float* out, int64_t ldo, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (hidden < 1 || hidden > 16384 || ldx < hidden || ldo < hidden) return hipErrorInvalidValue;
    if (!beta) {
        hipLaunchKernelGGL(score_gather_norm_kernel, dim3((unsigned)n), dim3(256), 0, stream, x, ldx, src, hidden, gamma, eps, out, ldo);
        return hipGetLastError();
    }
    // (the float4 form: 16-byte aligned rows on both sides)
    const bool v4 = hidden % 4 == 0 && hidden <= 256 * GN_V4_PER_LANE && ((ldx | ldo) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(gamma) |
                      reinterpret_cast<uintptr_t>(beta)) & 15) == 0;
    if (v4)
        hipLaunchKernelGGL(score_gather_layernorm_kernel<true>, dim3((unsigned)n), dim3(64), 0, stream, x, ldx, src, hidden, gamma, beta, eps, out,
                           ldo);
    else
        hipLaunchKernelGGL(score_gather_layernorm_kernel<false>, dim3((unsigned)n), dim3(64), 0, stream, x, ldx, src, hidden, gamma, beta, eps, out,
                           ldo);
    return hipGetLastError();
}

}  // namespace kjarni
