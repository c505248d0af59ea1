// The kernel of LlmModel::answer_logits_batch: a sequence's last hidden row through the final norm, then its dot products with
// the few head rows that were asked for -- the logits of those tokens without the vocabulary head.
//
//   RMSNorm     cpu/normalization/rms_norm.rs:19-27
//   LayerNorm   cpu/normalization/layer_norm.rs:96-131
//   lm head     a row of the (tied or untied) head per logit, f32 or bf16
#include "answer_logits_kernels.h"

#include "device_utils.h"
#include "dynamic_lds.h"

namespace kjarni {

namespace {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int AL_THREADS = 256, AL_WAVES = AL_THREADS / 64;
constexpr int AL_V4_PER_LANE = 4;  // (MAX_V4_PER_LANE of rowops.hip: hidden <= 1024 on launch_layernorm's float4 path)

enum { AL_RMS = 0, AL_LN_V4 = 1, AL_LN_GENERIC = 2 };

__device__ __forceinline__ float bf16_bits_to_float(unsigned short b) { return __uint_as_float((unsigned)b << 16); }

// One workgroup per sequence.  Wave 0 takes the row's statistic in the order of the kernel the layer stack would have used
// (rmsnorm_kernel: lane-strided fmaf chains, then the wave-wide butterfly, as score_gather_norm_kernel and last_token_pool_kernel
// follow it; layernorm_kernel's float4 registers and pairwise partial sums; layernorm_generic_kernel's passes), all four waves
// write the normalised row to LDS, then wave w takes targets w, w + 4: the head row is read once, 16 bytes per lane from its
// first 16-byte boundary on (the few elements in front of it and behind the last full vector one per lane), and a wave-wide
// sum gives the logit.  The statistics sit behind the row in the dynamic region (no static LDS in front of it).
template <int FORM, bool BF16>
__global__ __launch_bounds__(AL_THREADS) void answer_logits_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ src,
                                                                   int hidden, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps,
                                                                   const void* __restrict__ head, const uint32_t* __restrict__ targets,
                                                                   int n_targets, float* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) float al_smem[];
    float* sn = al_smem;                           // [hidden] the normalised row
    float* stat = al_smem + ((hidden + 3) & ~3);   // [2]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = x + (int64_t)src[b] * ldx;
    if (wave == 0) {
        if constexpr (FORM == AL_RMS) {
            float s = 0.0f;
            for (int i = lane; i < hidden; i += 64) s = fmaf(row[i], row[i], s);
            s = wave_sum(s);
            if (lane == 0) stat[0] = s;
        } else if constexpr (FORM == AL_LN_V4) {
            const int nv4 = hidden >> 2;
            f32x4 xr[AL_V4_PER_LANE];
#pragma unroll
            for (int i = 0; i < AL_V4_PER_LANE; ++i) {
                const int c4 = lane + i * 64;
                xr[i] = (c4 < nv4) ? *reinterpret_cast<const f32x4*>(row + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < AL_V4_PER_LANE; ++i)
                if (lane + i * 64 < nv4) s += (xr[i][0] + xr[i][1]) + (xr[i][2] + xr[i][3]);
            const float mean = wave_sum(s) / (float)hidden;
            float v = 0.0f;
#pragma unroll
            for (int i = 0; i < AL_V4_PER_LANE; ++i)
                if (lane + i * 64 < nv4) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float d = xr[i][c] - mean;
                        v = fmaf(d, d, v);
                    }
                }
            const float var = wave_sum(v) / (float)hidden;
            if (lane == 0) {
                stat[0] = mean;
                stat[1] = 1.0f / sqrtf(var + eps);
            }
        } else {
            float s = 0.f;
            for (int i = lane; i < hidden; i += 64) s += row[i];
            const float mean = wave_sum(s) / (float)hidden;
            float v = 0.f;
            for (int i = lane; i < hidden; i += 64) {
                const float d = row[i] - mean;
                v = fmaf(d, d, v);
            }
            const float inv_std = 1.0f / sqrtf(wave_sum(v) / (float)hidden + eps);
            if (lane == 0) {
                stat[0] = mean;
                stat[1] = inv_std;
            }
        }
    }
    __syncthreads();
    if constexpr (FORM == AL_RMS) {
        const float rms = sqrtf(stat[0] / (float)hidden + eps);
        for (int i = tid; i < hidden; i += AL_THREADS) sn[i] = (row[i] / rms) * gamma[i];
    } else {
        const float mean = stat[0], inv_std = stat[1];
        for (int i = tid; i < hidden; i += AL_THREADS) sn[i] = (row[i] - mean) * inv_std * gamma[i] + beta[i];
    }
    __syncthreads();
    for (int t = wave; t < n_targets; t += AL_WAVES) {
        float acc = 0.0f;
        if constexpr (BF16) {
            const unsigned short* w = static_cast<const unsigned short*>(head) + (int64_t)targets[t] * hidden;
            const int lead = min(hidden, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(w) & 15u)) & 15u) >> 1));
            const int nv = (hidden - lead) >> 3, tail = lead + nv * 8;
            if (lane < lead) acc = sn[lane] * bf16_bits_to_float(w[lane]);                       // (lead <= 7)
            if (tail + lane < hidden) acc = fmaf(sn[tail + lane], bf16_bits_to_float(w[tail + lane]), acc);  // (hidden - tail <= 7)
            for (int v = lane; v < nv; v += 64) {
                const u16x8 wv = *reinterpret_cast<const u16x8*>(w + lead + v * 8);
                const float* a = sn + lead + v * 8;
#pragma unroll
                for (int c = 0; c < 8; ++c) acc = fmaf(a[c], bf16_bits_to_float(wv[c]), acc);
            }
        } else {
            const float* w = static_cast<const float*>(head) + (int64_t)targets[t] * hidden;
            const int lead = min(hidden, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(w) & 15u)) & 15u) >> 2));
            const int nv = (hidden - lead) >> 2, tail = lead + nv * 4;
            if (lane < lead) acc = sn[lane] * w[lane];                                            // (lead <= 3)
            if (tail + lane < hidden) acc = fmaf(sn[tail + lane], w[tail + lane], acc);           // (hidden - tail <= 3)
            for (int v = lane; v < nv; v += 64) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + lead + v * 4);
                const float* a = sn + lead + v * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fmaf(a[c], wv[c], acc);
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) out[(int64_t)b * n_targets + t] = acc;
    }
}

}  // namespace

hipError_t launch_answer_logits(const float* x, int64_t ldx, const int32_t* src, int n, int hidden, const float* gamma, const float* beta,
                                float eps, const void* head, int head_is_bf16, const uint32_t* targets, int n_targets, float* out,
                                hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (hidden < 1 || hidden > 16384 || ldx < hidden || n_targets < 1 || n_targets > kAnswerMaxTargets) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(head) & (head_is_bf16 ? 1u : 3u)) != 0) return hipErrorInvalidValue;
    // (launch_layernorm's float4 form, where the row allows 16-byte loads)
    const bool v4 = beta && hidden % 4 == 0 && hidden <= 256 * AL_V4_PER_LANE && (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const int form = !beta ? AL_RMS : v4 ? AL_LN_V4 : AL_LN_GENERIC;
    const size_t lds = ((size_t)((hidden + 3) & ~3) + 4) * sizeof(float);
#define KJ_AL(FORM, BF)                                                                                                              \
    do {                                                                                                                             \
        auto kern = answer_logits_kernel<FORM, BF>;                                                                                  \
        if (lds > 48 * 1024) {                                                                                                       \
            const hipError_t e = allow_dynamic_lds(kern, lds);                                                                       \
            if (e != hipSuccess) return e;                                                                                           \
        }                                                                                                                            \
        hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(AL_THREADS), lds, stream, x, ldx, src, hidden, gamma, beta, eps, head, targets, \
                           n_targets, out);                                                                                          \
    } while (0)
    if (head_is_bf16) {
        if (form == AL_RMS) KJ_AL(AL_RMS, true);
        else if (form == AL_LN_V4) KJ_AL(AL_LN_V4, true);
        else KJ_AL(AL_LN_GENERIC, true);
    } else {
        if (form == AL_RMS) KJ_AL(AL_RMS, false);
        else if (form == AL_LN_V4) KJ_AL(AL_LN_V4, false);
        else KJ_AL(AL_LN_GENERIC, false);
    }
#undef KJ_AL
    return hipGetLastError();
}

}  // namespace kjarni
