// The scoring head on the bf16 matrix cores, for bf16 checkpoints (LlmModel::score_head with set_score_fused(2)): per row of the
// final-normed hidden states X[M, K] the log-softmax statistics of its N vocabulary logits X . W^T, the logits never stored.
//
// W [N, K] is bf16 in HBM and goes into LDS as it is: a bf16 weight is its own exact matrix-core operand.  X is f32 and becomes
// three bf16 planes on the way into LDS (sp_split, bf16_split.h: x = p1 + p2 + p3 exactly).  Per 16 columns of K a 32 x 32 tile
// takes three v_mfma_f32_32x32x16_bf16, the smallest plane first; every product is exact and the sums are f32, so this is the
// arithmetic of llm_score_head_kernel (llm_kernels.hip: bf16 widened to f32, v_mfma_f32_32x32x2_f32) in another summation order,
// with 3/8 of its matrix instructions and half of its weight bytes through LDS.
//
// The row state, the slab partials and the key lists are llm_score_head_kernel's (score_head_common.h), in its layout, so its
// merge kernels follow this kernel unchanged.  Its own translation unit because it is compiled with -fno-slp-vectorize, as
// gemm_split.hip is (the split's subtractions must not become packed f32 adds beside the MFMAs).
#include <hip/hip_runtime.h>

#include "bf16_split.h"
#include "device_utils.h"
#include "llm_kernels.h"
#include "score_head_common.h"

namespace kjarni {

namespace {

// Workgroup tile: 64 rows x 128 vocabulary columns (two of the slabs' 64-wide units), K in steps of 32.
constexpr int SB_BN = 2 * SC_BN, SB_BK = 32;
constexpr int SB_XPLANE = SC_BM * SB_BK;              // bf16 per X plane: 64 rows x 64 bytes
constexpr int SB_W = 3 * SB_XPLANE;                   // where the W tile begins in a stage
constexpr int SB_STAGE = SB_W + SB_BN * SB_BK;        // X1 | X2 | X3 | W: 10 240 bf16 = 20 KiB
static_assert(SC_TOPK * SC_BM * sizeof(unsigned long long) <= SB_STAGE * sizeof(uint16_t), "the key lists pass through one stage");

// One workgroup per (row tile, slab): 256 threads, four waves.  Wave (wv, wx) owns rows wx * 32 .. + 31 and, of every 128-column
// tile, the two 32-column sub-tiles j * 64 + wv * 32 (j = 0, 1): one X fragment (three planes) meets two W fragments, six MFMAs
// for five 16-byte LDS reads, and X is split once per 128 columns.  The product is the transposed tile W . X^T (A fragments
// from W, B fragments from X), so lane == row: a lane's 32 accumulators are 32 vocabulary entries of its own row.  LDS rows
// are 64 bytes, their four 16-byte chunks swizzled by (row >> 2) & 3 (prefill_gemm_bf16w_kernel's layout); two stages, the
// next K tile's global loads in flight under the MFMAs.  A slab is slab_tiles 64-column units: where that number is odd the
// slab's last tile is half a tile, and the fold masks columns >= the slab's end as it masks columns >= N (loads are clamped to
// row N - 1 of W).  Rows >= M load row M - 1 and are not stored.
template <int TOPK>
__global__ __launch_bounds__(256) void llm_score_head_bf16_kernel(const float* __restrict__ X, int64_t ldx, const uint16_t* __restrict__ W,
                                                                  const uint32_t* __restrict__ targets, int M, int N, int K, int m_tiles,
                                                                  int slab_tiles, int n_tiles, int slabs, ScorePartial* __restrict__ P)
{
    __shared__ __attribute__((aligned(16))) uint16_t sp[2][SB_STAGE];
    __shared__ ScorePartial sRed[SC_BM];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wv = wid >> 1, wx = wid & 1, l31 = lane & 31, half = lane >> 5;
    // XCD-aware order (llm_score_head_kernel's): every XCD takes one contiguous run of workgroups, row tiles fastest, so the
    // workgroups that stream the same slab of W sit behind the same L2
    const int64_t nwg = gridDim.x;
    const int64_t xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int64_t q8 = nwg / 8, r8 = nwg % 8;
    const int64_t bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + slot;
    const int mt = (int)(bid % m_tiles), slab = (int)(bid / m_tiles);
    const int m0 = mt * SC_BM;
    const int c_begin = slab * slab_tiles * SC_BN;
    const int c_end = min(min(slab * slab_tiles + slab_tiles, n_tiles) * SC_BN, N);  // the slab's columns: [c_begin, c_end)

    // X: 64 x 32 floats = 512 float4, two per thread, split into the planes.  W: 128 rows x 64 bytes = 512 chunks, two per thread.
    const int a_row = tid >> 3, a_c4 = tid & 7, b_row = tid >> 2, b_c = tid & 3;
    const float* x_ptr[2];
    int stX[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = a_row + 32 * i;
        x_ptr[i] = X + (int64_t)min(m0 + row, M - 1) * ldx + a_c4 * 4;
        stX[i] = row * SB_BK + (((a_c4 >> 1) ^ ((row >> 2) & 3)) * 2 + (a_c4 & 1)) * 4;
    }
    const int stW = SB_W + b_row * SB_BK + (b_c ^ ((b_row >> 2) & 3)) * 8;  // (rows b_row and b_row + 64 swizzle alike)
    const uint16_t* w_ptr[2];
    f32x4 gx[2];
    u32x4 gw[2];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) gx[i] = *reinterpret_cast<const f32x4*>(x_ptr[i] + k0);
#pragma unroll
        for (int i = 0; i < 2; ++i) gw[i] = *reinterpret_cast<const u32x4*>(w_ptr[i] + k0);
    };
    auto store = [&](int stage) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            u32x2 p1, p2, p3;
            sp_split(gx[i], p1, p2, p3);
            *reinterpret_cast<u32x2*>(&sp[stage][stX[i]]) = p1;
            *reinterpret_cast<u32x2*>(&sp[stage][SB_XPLANE + stX[i]]) = p2;
            *reinterpret_cast<u32x2*>(&sp[stage][2 * SB_XPLANE + stX[i]]) = p3;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(&sp[stage][stW + i * SC_BN * SB_BK]) = gw[i];
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
    const int nk = K / SB_BK;
    const int fsw = (l31 >> 2) & 3;
    const int fx = (wx * 32 + l31) * SB_BK, fw = SB_W + (wv * 32 + l31) * SB_BK;
    for (int n0 = c_begin; n0 < c_end; n0 += SB_BN) {
#pragma unroll
        for (int i = 0; i < 2; ++i) w_ptr[i] = W + (int64_t)min(n0 + b_row + SC_BN * i, N - 1) * K + b_c * 8;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
        load(0);
        store(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int cur = kt & 1;
            if (kt + 1 < nk) load((kt + 1) * SB_BK);
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const int ch = ((kb * 2 + half) ^ fsw) * 8;
                bf16x8 a[2], b[3];
#pragma unroll
                for (int j = 0; j < 2; ++j) a[j] = *reinterpret_cast<const bf16x8*>(&sp[cur][fw + j * SC_BN * SB_BK + ch]);
#pragma unroll
                for (int p = 0; p < 3; ++p) b[p] = *reinterpret_cast<const bf16x8*>(&sp[cur][p * SB_XPLANE + fx + ch]);
#pragma unroll
                for (int p = 2; p >= 0; --p)  // the smallest piece first; the two accumulators alternate
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[j], b[p], acc[j], 0, 0, 0);
            }
            if (kt + 1 < nk) store(cur ^ 1);
            __syncthreads();
        }
        // acc[j][r] = logit of (row, n0 + j * 64 + wv * 32 + acc_row(r, half)): fold the 32 into the lane's running state
        const int c0 = n0 + wv * 32;
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = c0 + j * SC_BN + acc_row(r, half);
                if (col < c_end) {
                    tmax = fmaxf(tmax, acc[j][r]);
                    const unsigned long long kk = argmax_key(acc[j][r], col);
                    if constexpr (TOPK > 0) topk_insert(lst, kk);
                    else key = kk > key ? kk : key;
                    if ((uint32_t)col == target) tgt = acc[j][r];
                }
            }
        if (tmax > -INFINITY) {
            const float nm = fmaxf(mx, tmax);
            float ts = 0.0f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (c0 + j * SC_BN + acc_row(r, half) < c_end) ts += expf(acc[j][r] - nm);
            sm = sm * expf(mx - nm) + ts;
            mx = nm;
        }
    }
    // the two half-waves of a row, then the two waves (llm_score_head_kernel's order)
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
    // [TOPK][SC_BM] keys through the first stage, which nobody reads after the last tile's closing barrier
    [[maybe_unused]] unsigned long long* sKeys = reinterpret_cast<unsigned long long*>(&sp[0][0]);
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

}  // namespace

bool llm_score_head_bf16_takes(const float* X, int64_t ldx, const void* W, int k)
{
    return k > 0 && k % SB_BK == 0 && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
}

hipError_t launch_score_head_bf16(const float* X, int64_t ldx, int m, const void* W, int vocab, int k, const uint32_t* targets, int slab_tiles,
                                  void* scratch, float* logprob, uint32_t* top, float* top_logprob, float* lse, hipStream_t stream)
{
    if (m <= 0) return hipSuccess;
    if (vocab <= 0 || !scratch || !llm_score_head_bf16_takes(X, ldx, W, k)) return hipErrorInvalidValue;
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    const int st = score_head_slab_tiles(m, vocab, slab_tiles);
    const int slabs = (n_tiles + st - 1) / st;
    ScorePartial* P = static_cast<ScorePartial*>(scratch);
    hipLaunchKernelGGL(llm_score_head_bf16_kernel<0>, dim3((unsigned)(m_tiles * slabs)), dim3(256), 0, stream, X, ldx,
                       static_cast<const uint16_t*>(W), targets, m, vocab, k, m_tiles, st, n_tiles, slabs, P);
    return launch_score_merge(P, targets, m, vocab, slabs, st, logprob, top, top_logprob, lse, stream);
}

hipError_t launch_score_head_bf16_topk(const float* X, int64_t ldx, int m, const void* W, int vocab, int k, const uint32_t* targets,
                                       int slab_tiles, int top_k, void* scratch, float* logprob, uint32_t* topk_ids, float* topk_logprob,
                                       float* lse, hipStream_t stream)
{
    if (m <= 0) return hipSuccess;
    if (vocab <= 0 || top_k < 1 || top_k > SC_TOPK || top_k > vocab || !scratch || !llm_score_head_bf16_takes(X, ldx, W, k))
        return hipErrorInvalidValue;
    const int n_tiles = (vocab + SC_BN - 1) / SC_BN, m_tiles = (m + SC_BM - 1) / SC_BM;
    const int st = score_head_slab_tiles(m, vocab, slab_tiles);
    const int slabs = (n_tiles + st - 1) / st;
    ScorePartial* P = static_cast<ScorePartial*>(scratch);
    const unsigned long long* PK = reinterpret_cast<const unsigned long long*>(P + (int64_t)m_tiles * slabs * SC_BM);  // where the kernel writes
    float* row_lse = lse ? lse : const_cast<float*>(reinterpret_cast<const float*>(PK + (int64_t)m_tiles * slabs * SC_TOPK * SC_BM));
    hipLaunchKernelGGL(llm_score_head_bf16_kernel<SC_TOPK>, dim3((unsigned)(m_tiles * slabs)), dim3(256), 0, stream, X, ldx,
                       static_cast<const uint16_t*>(W), targets, m, vocab, k, m_tiles, st, n_tiles, slabs, P);
    // logprob and lse by the merge of the call without top-k, in its order; then the lists
    const hipError_t e = launch_score_merge(P, targets, m, vocab, slabs, st, logprob, nullptr, nullptr, row_lse, stream);
    return e != hipSuccess ? e : launch_score_topk_merge(PK, row_lse, m, slabs, top_k, topk_ids, topk_logprob, stream);
}

}  // namespace kjarni
