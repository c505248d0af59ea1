// Kernels of the decoder embedders: the packed-row counterparts of the prompt kernels in llm_kernels.hip.  A chunk holds the
// rows of several sequences one after another; attention stops at the sequence boundaries, RoPE takes each row's position
// inside its own sequence, and the pool reads each sequence's last row.
//
//   attention   cpu/decoder/decoder_attention.rs:99-160, utils/masks.rs:103-113 (per sequence)
//   RoPE        cpu/rope/mod.rs:156-176
//   RMSNorm     cpu/normalization/rms_norm.rs:19-27
//   last token  pooling/mod.rs:61-62; L2: cpu/encoder/traits.rs:529-536
#include <algorithm>

#include "decoder_embed_kernels.h"
#include "device_utils.h"
#include "dynamic_lds.h"

namespace kjarni {

namespace {

// prefill_attention_kernel (llm_kernels.hip) on one query block of one packed sequence: the sequence's rows are the whole
// "cache" (base = 0), so keys and queries are clamped inside it.  32 queries x 64-key tiles, 8 threads per query, running
// (max, sum, output) per query.  A query's masked keys are left out of its sums (the P V loop ends at its last visible key).
constexpr int PK_Q = 32, PK_K = 64;

template <int DPT>
__global__ __launch_bounds__(256) void packed_attention_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ K,
                                                               int64_t ldk, const float* __restrict__ V, int64_t ldv,
                                                               const EmbedBlock* __restrict__ blocks, int kv_group, float scale,
                                                               float* __restrict__ ctx, int64_t ldc)
{
    constexpr int D = 8 * DPT, LD = D + 4;
    extern __shared__ __attribute__((aligned(16))) float pk_smem[];
    float* sQ = pk_smem;               // [PK_Q][LD]
    float* sK = sQ + PK_Q * LD;        // [PK_K][LD]
    float* sV = sK + PK_K * LD;        // [PK_K][LD]
    float* sP = sV + PK_K * LD;        // [PK_Q][PK_K + 4]
    const EmbedBlock eb = blocks[blockIdx.x];
    const int rows = eb.len, q0 = eb.q0;
    q += (int64_t)eb.first * ldq;
    K += (int64_t)eb.first * ldk;
    V += (int64_t)eb.first * ldv;
    ctx += (int64_t)eb.first * ldc;
    const int tid = threadIdx.x, qi = tid >> 3, kg = tid & 7;
    const int h = blockIdx.y, hk = h / kv_group;
    const int q_row = q0 + qi;
    const bool valid = q_row < rows;
    const int limit = q_row;                                 // last visible key of this query
    const int last_key = min(rows, q0 + PK_Q) - 1;           // last key any query of the block sees
    for (int i = tid; i < PK_Q * (D / 4); i += 256) {
        const int r = i / (D / 4), c4 = i - r * (D / 4);
        const int row = min(q0 + r, rows - 1);
        *reinterpret_cast<f32x4*>(sQ + r * LD + c4 * 4) = *reinterpret_cast<const f32x4*>(q + (int64_t)row * ldq + h * D + c4 * 4);
    }
    float m_run = -INFINITY, l_run = 0.0f;
    float o[DPT];
#pragma unroll
    for (int c = 0; c < DPT; ++c) o[c] = 0.0f;
    for (int k0 = 0; k0 <= last_key; k0 += PK_K) {
        __syncthreads();  // previous tile fully consumed (and sQ written, first trip)
        for (int i = tid; i < PK_K * (D / 4); i += 256) {
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
            sP[qi * (PK_K + 4) + kg + 8 * j] = p;
        }
        psum = group8_sum_asc(psum);
        const float alpha = (m_new == -INFINITY || m_run == -INFINITY) ? (m_run == -INFINITY ? 0.0f : 1.0f) : expf(m_run - m_new);
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int c = 0; c < DPT; ++c) o[c] *= alpha;
        m_run = m_new;
        __syncthreads();  // the tile's probabilities are in LDS
        const int jn = valid ? min(PK_K, limit - k0 + 1) : 0;  // the tile's keys this query sees
        for (int j = 0; j < jn; ++j) {
            const float p = sP[qi * (PK_K + 4) + j];
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

// prefill_attention_mfma_kernel (llm_kernels.hip) on one 128-query block of one packed sequence (base = 0): 4 waves x 32
// queries, 128-key chunks staged in LDS (K row-major, V transposed), S^T = K Q^T and O += P V as 32 x 32 x 2 MFMA tiles, online
// softmax in the exp2 domain.  Keys at or past the sequence's length are staged as zeros and never loaded.
constexpr int PKM_Q = 128, PKM_K = 128;
template <int D>
struct PkmSmem {
    static constexpr int K_STRIDE = D + 4, VT_STRIDE = PKM_K + 4;
    static constexpr int K_FLOATS = PKM_K * K_STRIDE, VT_FLOATS = D * VT_STRIDE;
    static constexpr int BYTES = (K_FLOATS + VT_FLOATS) * 4;
};

template <int D>
__global__ __launch_bounds__(256, D <= 64 ? 2 : 1) void packed_attention_mfma_kernel(const float* __restrict__ q, int64_t ldq,
                                                                                      const float* __restrict__ K, int64_t ldk,
                                                                                      const float* __restrict__ V, int64_t ldv,
                                                                                      const EmbedBlock* __restrict__ blocks, int kv_group,
                                                                                      float scale, float* __restrict__ ctx, int64_t ldc)
{
    using SM = PkmSmem<D>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sK = smem;                  // [128][D + 4]
    float* sVt = smem + SM::K_FLOATS;  // [D][128 + 4]
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    // A query block's work grows with its index inside its sequence: the upper half of the heads walks the table in reverse, so
    // that the workgroups that tend to share a CU add up to the same work.
    const int h = blockIdx.y, kvh = h / kv_group;
    const int entry = (2 * (int)blockIdx.y >= (int)gridDim.y) ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const EmbedBlock eb = blocks[entry];
    const int rows = eb.len;
    const float* q_base = q + (int64_t)eb.first * ldq + h * D;
    const float* k_base = K + (int64_t)eb.first * ldk + kvh * D;
    const float* v_base = V + (int64_t)eb.first * ldv + kvh * D;

    const int q_wave0 = eb.q0 + wid * 32;  // first query row of this wave
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
    const int n_keys = rows;
    const int last_q_wg = min(rows, eb.q0 + PKM_Q) - 1;        // last query row of the workgroup
    const int last_q_wave = min(rows - 1, q_wave0 + 31);        // (below q_wave0 when the wave has no query: it only helps staging)
    const int n_chunks = last_q_wg / PKM_K + 1;
    const float c1 = scale * 1.4426950408889634f;

    for (int ch = 0; ch < n_chunks; ++ch) {
        const int key0 = ch * PKM_K;
        if (ch > 0) __syncthreads();  // everyone done reading the previous chunk
        constexpr int V4_PER_ROW = D / 4;
        for (int f = tid; f < PKM_K * V4_PER_ROW; f += 256) {
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
        if (q_wave0 >= rows || key0 > last_q_wave) continue;  // no query here, or every key of the chunk is in this wave's future
        const bool plain = key0 + PKM_K - 1 <= q_wave0;      // every key visible to every query of the wave

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
            const int limit = q_row;  // this lane's query sees keys <= limit
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
    float* out_base = ctx + (int64_t)eb.first * ldc + h * D;
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

// rope_kernel (llm_kernels.hip) with the position of row r read from row_pos[r].
__global__ __launch_bounds__(256) void rope_rows_kernel(float* __restrict__ x, int64_t ldx, int rows, int n_heads, int head_dim,
                                                        const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                        const int32_t* __restrict__ row_pos)
{
    const int half = head_dim >> 1;
    const int total = rows * n_heads * half;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int i = idx % half;
        const int h = (idx / half) % n_heads;
        const int r = idx / (half * n_heads);
        const int p = row_pos[r];
        float* row = x + (int64_t)r * ldx + h * head_dim;
        const float c = cos_t[(int64_t)p * half + i], s = sin_t[(int64_t)p * half + i];
        const float x0 = row[i], x1 = row[i + half];
        row[i] = x0 * c - x1 * s;
        row[i + half] = x0 * s + x1 * c;
    }
}

// qk_norm_rope_kernel (llm_kernels.hip) with the position of row r read from row_pos[r]: one wave per head, RMS statistic of
// the head reduced across the wave, normalised, scaled by gamma, rotated.
__global__ __launch_bounds__(256) void qk_norm_rope_rows_kernel(float* __restrict__ q, int64_t ldq, float* __restrict__ k, int64_t ldk,
                                                                int rows, int n_heads, int n_kv_heads, int head_dim,
                                                                const float* __restrict__ gamma_q, const float* __restrict__ gamma_k,
                                                                float eps, const float* __restrict__ cos_t,
                                                                const float* __restrict__ sin_t, const int32_t* __restrict__ row_pos)
{
    const int lane = threadIdx.x & 63;
    const int per_row = n_heads + n_kv_heads;
    const int job = blockIdx.x * 4 + (threadIdx.x >> 6);  // uniform over the wave
    if (job >= rows * per_row) return;
    const int r = job / per_row, h = job - r * per_row;
    const int p = row_pos[r];
    const bool is_q = h < n_heads;
    float* x = is_q ? q + (int64_t)r * ldq + h * head_dim : k + (int64_t)r * ldk + (h - n_heads) * head_dim;
    const float* gamma = is_q ? gamma_q : gamma_k;
    const int half = head_dim >> 1;
    const bool on = lane < half;
    const float x0 = on ? x[lane] : 0.0f, x1 = on ? x[lane + half] : 0.0f;
    float s = fmaf(x0, x0, 0.0f);
    s = fmaf(x1, x1, s);
    const float rms = sqrtf(wave_sum(s) / (float)head_dim + eps);  // every lane of the wave is here: the reduction is wave-wide
    if (!on) return;
    const float y0 = (x0 / rms) * gamma[lane], y1 = (x1 / rms) * gamma[lane + half];
    const float c = cos_t[(int64_t)p * half + lane], sn = sin_t[(int64_t)p * half + lane];
    x[lane] = y0 * c - y1 * sn;
    x[lane + half] = y0 * sn + y1 * c;
}

// One workgroup per sequence: its last row through the final RMSNorm (the statistic summed as rmsnorm_kernel sums it: lane-strided
// fmaf chains of one wave, then the wave-wide butterfly) and the optional L2 normalisation.
__global__ __launch_bounds__(256) void last_token_pool_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ seq_start,
                                                              int hidden, const float* __restrict__ gamma, float eps, int normalize,
                                                              float* __restrict__ out)
{
    __shared__ float red[5];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = x + (int64_t)(seq_start[b + 1] - 1) * ldx;
    if (wave == 0) {
        float s = 0.0f;
        for (int i = lane; i < hidden; i += 64) s = fmaf(row[i], row[i], s);
        s = wave_sum(s);
        if (lane == 0) red[4] = s;
    }
    __syncthreads();
    const float rms = sqrtf(red[4] / (float)hidden + eps);
    float sq = 0.0f;
    for (int i = tid; i < hidden; i += 256) {
        const float y = (row[i] / rms) * gamma[i];
        sq = fmaf(y, y, sq);
    }
    float norm = 0.0f;
    if (normalize) {
        sq = wave_sum(sq);
        if (lane == 0) red[wave] = sq;
        __syncthreads();
        norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    }
    for (int i = tid; i < hidden; i += 256) {
        float y = (row[i] / rms) * gamma[i];
        if (norm > 0.0f) y = y / norm;  // traits.rs:529-536: divide only when the norm is > 0
        out[(int64_t)b * hidden + i] = y;
    }
}

}  // namespace

hipError_t launch_packed_causal_attention(const float* q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                                          const EmbedBlock* vec, int n_vec, const EmbedBlock* mfma, int n_mfma, int heads, int head_dim,
                                          int kv_group, float* ctx, int64_t ldc, hipStream_t stream)
{
    if (n_vec <= 0 && n_mfma <= 0) return hipSuccess;
    if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
    if (heads < 1 || ((ldq | ldk | ldv | ldc) & 3) != 0 ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(K) | reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(ctx)) & 15) != 0)
        return hipErrorInvalidValue;
    if (n_mfma > 0 && head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
    const int g = kv_group < 1 ? 1 : kv_group;
    const float scale = 1.0f / sqrtf((float)head_dim);
    if (n_mfma > 0) {
        const dim3 mgrid((unsigned)n_mfma, (unsigned)heads);
        if (head_dim == 64) {
            auto kern = packed_attention_mfma_kernel<64>;
            const hipError_t e = allow_dynamic_lds(kern, PkmSmem<64>::BYTES);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, mgrid, dim3(256), PkmSmem<64>::BYTES, stream, q, ldq, K, ldk, V, ldv, mfma, g, scale, ctx, ldc);
        } else {
            auto kern = packed_attention_mfma_kernel<128>;
            const hipError_t e = allow_dynamic_lds(kern, PkmSmem<128>::BYTES);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, mgrid, dim3(256), PkmSmem<128>::BYTES, stream, q, ldq, K, ldk, V, ldv, mfma, g, scale, ctx, ldc);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n_vec <= 0) return hipSuccess;
    const dim3 grid((unsigned)n_vec, (unsigned)heads);
    const int LD = head_dim + 4;
    const size_t lds = ((size_t)(PK_Q + 2 * PK_K) * LD + (size_t)PK_Q * (PK_K + 4)) * sizeof(float);
#define KJ_PK(DPT)                                                                                                       \
    do {                                                                                                                 \
        auto kern = packed_attention_kernel<DPT>;                                                                        \
        if (lds > 48 * 1024) {                                                                                           \
            const hipError_t e = allow_dynamic_lds(kern, lds);                                                           \
            if (e != hipSuccess) return e;                                                                               \
        }                                                                                                                \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, q, ldq, K, ldk, V, ldv, vec, g, scale, ctx, ldc);         \
    } while (0)
    switch (head_dim) {
    case 16: KJ_PK(2); break;
    case 32: KJ_PK(4); break;
    case 64: KJ_PK(8); break;
    default: KJ_PK(16); break;
    }
#undef KJ_PK
    return hipGetLastError();
}

hipError_t launch_rope_rows(float* x, int64_t ldx, int rows, int n_heads, int head_dim, const float* cos_t, const float* sin_t,
                            const int32_t* row_pos, hipStream_t stream)
{
    const int64_t total = (int64_t)rows * n_heads * (head_dim / 2);
    if (total <= 0) return hipSuccess;
    if (total > (int64_t)1 << 30) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rope_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, x, ldx, rows, n_heads, head_dim, cos_t,
                       sin_t, row_pos);
    return hipGetLastError();
}

hipError_t launch_qk_norm_rope_rows(float* q, int64_t ldq, float* k, int64_t ldk, int rows, int n_heads, int n_kv_heads, int head_dim,
                                    const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                    const int32_t* row_pos, hipStream_t stream)
{
    if (rows <= 0 || n_heads + n_kv_heads <= 0) return hipSuccess;
    if (n_heads < 0 || n_kv_heads < 0 || head_dim < 2 || head_dim > 128 || (head_dim & 1)) return hipErrorInvalidValue;
    const int64_t jobs = (int64_t)rows * (n_heads + n_kv_heads);
    if (jobs > (int64_t)1 << 30) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qk_norm_rope_rows_kernel, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, stream, q, ldq, k, ldk, rows, n_heads,
                       n_kv_heads, head_dim, gamma_q, gamma_k, eps, cos_t, sin_t, row_pos);
    return hipGetLastError();
}

hipError_t launch_last_token_pool(const float* x, int64_t ldx, const int32_t* seq_start, int n_seq, int hidden, const float* gamma, float eps,
                                  int normalize, float* out, hipStream_t stream)
{
    if (n_seq <= 0) return hipSuccess;
    if (hidden < 1 || hidden > 16384 || ldx < hidden) return hipErrorInvalidValue;
    hipLaunchKernelGGL(last_token_pool_kernel, dim3((unsigned)n_seq), dim3(256), 0, stream, x, ldx, seq_start, hidden, gamma, eps, normalize,
                       out);
    return hipGetLastError();
}

}  // namespace kjarni
