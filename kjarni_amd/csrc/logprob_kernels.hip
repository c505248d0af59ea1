// Generation log-probabilities (logprob_kernels.h): the slab pass over a step's logits rows and the merge that writes the record.
#include "logprob_kernels.h"

#include <algorithm>

namespace kjarni {

namespace {

constexpr int kWave = 64;
constexpr int LP_THREADS = 256, LP_STEP = LP_THREADS * 4;  // elements a workgroup takes per trip: one 16-byte load per thread
typedef float lp_f32x4 __attribute__((ext_vector_type(4)));

// launch_argmax's key (llm_kernels.hip: argmax_key), restated: larger float -> larger key, NaN lowest, -0.0 == +0.0, and among
// equal values the later index wins.  tests/test_gpu_gen_logprobs.py holds slot 0 against kjarni_hip_op_argmax bit for bit.
__device__ __forceinline__ unsigned long long lp_key(float v, int idx)
{
    uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (v != v) u = 0;
    return ((unsigned long long)u << 32) | (uint32_t)idx;
}

__device__ __forceinline__ float lp_key_value(unsigned long long key)
{
    const uint32_t u = (uint32_t)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// (mx, sm) += (omx, osm): sums of exp(x - mx) brought to the common maximum.  The two lanes of a butterfly pair evaluate it with
// the sides swapped, and under -ffp-contract=on the sum of two products may round differently on each side: whoever needs one
// value for the whole wave takes lane 0's (the slab pass stores lane 0's; the finish kernel broadcasts lane 0's lse).
__device__ __forceinline__ void lp_combine(float& mx, float& sm, float omx, float osm)
{
    const float m = fmaxf(mx, omx);
    if (m == -INFINITY) return;  // both empty
    sm = sm * expf(mx - m) + osm * expf(omx - m);
    mx = m;
}

// A list of TOPK keys in descending order, every index static so that it lives in registers; 0 marks an empty slot.  Keys of
// different columns differ, so "the TOPK largest keys" is one set whatever the order of the insertions.
template <int TOPK>
__device__ __forceinline__ void lp_insert(unsigned long long (&lst)[TOPK], unsigned long long kk)
{
    if (kk > lst[TOPK - 1]) {  // the one compare of the common path
#pragma unroll
        for (int j = TOPK - 1; j > 0; --j) lst[j] = kk > lst[j - 1] ? lst[j - 1] : (kk > lst[j] ? kk : lst[j]);
        lst[0] = kk > lst[0] ? kk : lst[0];
    }
}

// The largest key of the wave, in every lane (butterfly; integer compares: every lane ends with the same key).
__device__ __forceinline__ unsigned long long lp_wave_max(unsigned long long key)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, kWave);
        key = o > key ? o : key;
    }
    return key;
}

// lst (descending in every lane) = the TOPK largest keys of all the wave's lists, descending, in every lane: TOPK times the
// largest head of the wave is taken and popped from the one lane that holds it (keys of different columns differ).  Merging whole
// lists lane by lane costs TOPK inserts per butterfly step; this costs one 64-bit maximum per slot.
template <int TOPK>
__device__ __forceinline__ void lp_wave_topk(unsigned long long (&lst)[TOPK])
{
    unsigned long long out[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) {
        const unsigned long long best = lp_wave_max(lst[0]);
        out[j] = best;
        if (lst[0] == best && best != 0ull) {
#pragma unroll
            for (int i = 0; i + 1 < TOPK; ++i) lst[i] = lst[i + 1];
            lst[TOPK - 1] = 0ull;
        }
    }
#pragma unroll
    for (int j = 0; j < TOPK; ++j) lst[j] = out[j];
}

struct LpSlab {
    float mx, sm;
};

// Slab blockIdx.x of row blockIdx.y.  A thread walks its own elements in index order (four consecutive ones per trip) with a
// running maximum, the sum of exp(x - max) rescaled when the maximum moves, and its TOPK largest keys; then lane -> wave
// (butterfly for the sums, lp_wave_topk for the lists) -> workgroup (the four waves through LDS: the sums in wave order by thread 0,
// the lists by the first wave).  vec: the rows (and the copy's) are 16-byte aligned with
// a pitch that is a multiple of 4, so a trip is one 16-byte load; the element-wise trips of the other case, and of the last
// slab's tail, see the same elements in the same order.
template <int TOPK>
__global__ __launch_bounds__(LP_THREADS) void token_logprob_partial_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int slab_len,
                                                                           int vec, const int32_t* __restrict__ live,
                                                                           LpSlab* __restrict__ stats, unsigned long long* __restrict__ keys,
                                                                           float* __restrict__ raw_copy, int64_t ld_copy)
{
    __shared__ float red_mx[4], red_sm[4];
    __shared__ unsigned long long red_key[4 * TOPK];
    const int r = blockIdx.y, slab = blockIdx.x, slabs = gridDim.x;
    if (live && !live[r]) return;  // (uniform per workgroup, before the barrier)
    const int begin = slab * slab_len, end = min(begin + slab_len, vocab);
    const float* row = logits + (int64_t)r * ld;
    float* copy = raw_copy ? raw_copy + (int64_t)r * ld_copy : nullptr;
    float mx = -INFINITY, sm = 0.0f;
    unsigned long long lst[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) lst[j] = 0ull;
    for (int i = begin + (int)threadIdx.x * 4; i < end; i += LP_STEP) {
        const int n = min(4, end - i);
        float x[4];
        if (vec && n == 4) {
            const lp_f32x4 v = *reinterpret_cast<const lp_f32x4*>(row + i);
            if (copy) *reinterpret_cast<lp_f32x4*>(copy + i) = v;
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[j] = j < n ? row[i + j] : -INFINITY;
                if (copy && j < n) copy[i + j] = x[j];
            }
        }
        const float m4 = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
        if (m4 > mx) {
            sm *= expf(mx - m4);  // (mx == -inf: sm is 0 and stays 0)
            mx = m4;
        }
        if (mx != -INFINITY) sm += (expf(x[0] - mx) + expf(x[1] - mx)) + (expf(x[2] - mx) + expf(x[3] - mx));
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) lp_insert(lst, lp_key(x[j], i + j));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float omx = __shfl_xor(mx, off, kWave), osm = __shfl_xor(sm, off, kWave);
        lp_combine(mx, sm, omx, osm);
    }
    lp_wave_topk(lst);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_mx[wave] = mx;
        red_sm[wave] = sm;
#pragma unroll
        for (int j = 0; j < TOPK; ++j) red_key[wave * TOPK + j] = lst[j];
    }
    __syncthreads();
    if (threadIdx.x >= kWave) return;
    // the first wave: lane l takes key l of the four waves' lists as a list of one, and the TOPK largest are popped as above
    unsigned long long one[1] = {threadIdx.x < 4 * TOPK ? red_key[threadIdx.x] : 0ull};
#pragma unroll
    for (int j = 0; j < TOPK; ++j) {
        lst[j] = lp_wave_max(one[0]);
        if (one[0] == lst[j]) one[0] = 0ull;
    }
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w) lp_combine(mx, sm, red_mx[w], red_sm[w]);
    const int64_t at = (int64_t)r * slabs + slab;
    stats[at] = LpSlab{mx, sm};
#pragma unroll
    for (int j = 0; j < TOPK; ++j) keys[at * kLogprobTopkMax + j] = lst[j];
}

// One wave per row: lane l holds slab l (slabs <= 64); the butterfly over (max, sum) and lp_wave_topk over the lists leave the
// row's list in every lane and its sums in lane 0's order -- one order, whatever the launch.  Lane 0 writes logprob and lse, lane j < top_k slot j.
template <int TOPK>
__global__ __launch_bounds__(kWave) void token_logprob_finish_kernel(const LpSlab* __restrict__ stats, const unsigned long long* __restrict__ keys,
                                                                     int slabs, int vocab, int top_k, const int32_t* __restrict__ live,
                                                                     const float* __restrict__ raw, int64_t ld_raw,
                                                                     const int32_t* __restrict__ tokens, int token_stride,
                                                                     const int* __restrict__ count, int count_stride, int index_bias,
                                                                     int rec_stride, int rec_cap, int slots, float* __restrict__ logprob,
                                                                     uint32_t* __restrict__ topk_ids, float* __restrict__ topk_logprob,
                                                                     float* __restrict__ lse_out)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    if (live && !live[r]) return;  // (the whole wave)
    float mx = -INFINITY, sm = 0.0f;
    unsigned long long lst[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) lst[j] = 0ull;
    if (lane < slabs) {
        const int64_t at = (int64_t)r * slabs + lane;
        const LpSlab s = stats[at];
        mx = s.mx;
        sm = s.sm;
#pragma unroll
        for (int j = 0; j < TOPK; ++j) lst[j] = keys[at * kLogprobTopkMax + j];  // (descending, as the slab pass left them)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float omx = __shfl_xor(mx, off, kWave), osm = __shfl_xor(sm, off, kWave);
        lp_combine(mx, sm, omx, osm);
    }
    lp_wave_topk(lst);
    const float lse = __shfl(mx + logf(sm), 0, kWave);  // one lse for logprob, lse and every slot
    const int32_t token = tokens ? tokens[(int64_t)r * token_stride] : (int32_t)(uint32_t)(lst[0] & 0xFFFFFFFFull);
    if (token < 0 || token >= vocab) return;
    const int idx = (count ? count[(int64_t)r * count_stride] : 0) + index_bias;
    if (idx < 0 || idx >= rec_cap) return;
    const int64_t at = (int64_t)r * rec_stride + idx;
    if (lane == 0) {
        if (logprob) logprob[at] = raw[(int64_t)r * ld_raw + token] - lse;
        if (lse_out) lse_out[at] = lse;
    }
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < TOPK; ++j) mine = lane == j ? lst[j] : mine;
    if (lane < top_k) {
        if (topk_ids) topk_ids[at * slots + lane] = (uint32_t)(mine & 0xFFFFFFFFull);
        if (topk_logprob) topk_logprob[at * slots + lane] = lp_key_value(mine) - lse;
    }
}

bool args_ok(const TokenLogprobArgs& a)
{
    return a.logits && a.scratch && a.rows >= 1 && a.rows <= kLogprobMaxRows && a.vocab >= 1 && a.ld >= a.vocab && a.top_k >= 0 &&
           a.top_k <= kLogprobTopkMax && a.top_k <= a.vocab && (!a.raw_copy || a.ld_copy >= a.vocab);
}

bool aligned16(const void* p, int64_t pitch) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && pitch % 4 == 0; }

}  // namespace

int token_logprob_slab_len(int rows, int vocab)
{
    if (rows < 1 || vocab < 1) return 0;
    const int by_width = (vocab + kLogprobMinSlab - 1) / kLogprobMinSlab, by_grid = std::max(1, (kLogprobGridTarget + rows - 1) / rows);
    const int want = std::min(kLogprobMaxSlabs, std::min(by_width, by_grid));
    return ((vocab + want - 1) / want + 3) / 4 * 4;
}

int token_logprob_slabs(int rows, int vocab)
{
    const int len = token_logprob_slab_len(rows, vocab);
    return len ? (vocab + len - 1) / len : 0;
}

size_t token_logprob_scratch_bytes(int rows, int vocab)
{
    if (rows < 1 || vocab < 1) return 0;
    return (size_t)rows * kLogprobMaxSlabs * (sizeof(LpSlab) + kLogprobTopkMax * sizeof(unsigned long long));
}

// The two halves of the scratch: the (max, sum) pairs of every (row, slab), then their key lists.
static LpSlab* scratch_stats(const TokenLogprobArgs& a) { return static_cast<LpSlab*>(a.scratch); }
static unsigned long long* scratch_keys(const TokenLogprobArgs& a)
{
    return reinterpret_cast<unsigned long long*>(scratch_stats(a) + (size_t)a.rows * kLogprobMaxSlabs);
}

hipError_t launch_token_logprob_partial(const TokenLogprobArgs& a, hipStream_t stream)
{
    if (!args_ok(a)) return hipErrorInvalidValue;
    const int len = token_logprob_slab_len(a.rows, a.vocab), slabs = token_logprob_slabs(a.rows, a.vocab);
    const int vec = aligned16(a.logits, a.ld) && (!a.raw_copy || aligned16(a.raw_copy, a.ld_copy)) ? 1 : 0;
    const dim3 grid((unsigned)slabs, (unsigned)a.rows);
    if (a.top_k <= 1)
        hipLaunchKernelGGL(token_logprob_partial_kernel<1>, grid, dim3(LP_THREADS), 0, stream, a.logits, a.ld, a.vocab, len, vec, a.live,
                           scratch_stats(a), scratch_keys(a), a.raw_copy, a.ld_copy);
    else
        hipLaunchKernelGGL(token_logprob_partial_kernel<kLogprobTopkMax>, grid, dim3(LP_THREADS), 0, stream, a.logits, a.ld, a.vocab, len, vec,
                           a.live, scratch_stats(a), scratch_keys(a), a.raw_copy, a.ld_copy);
    return hipGetLastError();
}

hipError_t launch_token_logprob_finish(const TokenLogprobArgs& a, const TokenLogprobRecord& rec, hipStream_t stream)
{
    if (!args_ok(a) || !rec.raw || rec.ld_raw < a.vocab || rec.rec_cap < 1 || rec.slots < a.top_k) return hipErrorInvalidValue;
    const int slabs = token_logprob_slabs(a.rows, a.vocab);
    if (a.top_k <= 1)
        hipLaunchKernelGGL(token_logprob_finish_kernel<1>, dim3((unsigned)a.rows), dim3(kWave), 0, stream, scratch_stats(a), scratch_keys(a), slabs,
                           a.vocab, a.top_k, a.live, rec.raw, rec.ld_raw, rec.tokens, rec.token_stride, rec.count, rec.count_stride,
                           rec.index_bias, rec.rec_stride, rec.rec_cap, rec.slots, rec.logprob, rec.topk_ids, rec.topk_logprob, rec.lse);
    else
        hipLaunchKernelGGL(token_logprob_finish_kernel<kLogprobTopkMax>, dim3((unsigned)a.rows), dim3(kWave), 0, stream, scratch_stats(a),
                           scratch_keys(a), slabs, a.vocab, a.top_k, a.live, rec.raw, rec.ld_raw, rec.tokens, rec.token_stride, rec.count,
                           rec.count_stride, rec.index_bias, rec.rec_stride, rec.rec_cap, rec.slots, rec.logprob, rec.topk_ids,
                           rec.topk_logprob, rec.lse);
    return hipGetLastError();
}

}  // namespace kjarni
