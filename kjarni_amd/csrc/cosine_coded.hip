// Cosine search over an int8 companion plane of the corpus, exact results.
//
// The many-query search of cosine.hip keeps the documents that can matter with a cheap pass of KNOWN error and decides them with
// cosine_rescore_kernel; that pass still streams the f32 corpus.  Here the cheap pass reads ONE byte per element: beside the f32
// rows an index keeps, per document d, codes c in [-127, 127]^dim (int8) with the scale s = max|d_i| / 127, so that d = s c + r,
// and three floats: s, e >= ||r|| (rounded up) and ||d|| (f32, the streaming scan's arithmetic).  A query is encoded the same way
// per call, q = s_q c_q + r_q.  Then
//       q.d - s_q s (c_q.c)  =  (s_q c_q).r + r_q.d          and, by Cauchy-Schwarz twice,
//     | q.d - s_q s (c_q.c) | <=  ||s_q c_q|| e + ||r_q|| ||d||  <=  (||q|| + e_q) e + e_q ||d||  =: B(q, d).
// c_q.c is an exact integer (|c_q.c| <= 1024 x 127^2 < 2^24: exact in i32 and in its conversion to f32), so what is left is f32
// rounding, covered by ONE relative slack kappa on ||q|| ||d||:
//   * forming s_q (s I) + a_q e + w_q ||d|| (two multiplies, two fmas; the sample's form has a reciprocal pair more): each
//     rounding is 2^-24 of a partial sum of magnitude < 2.6 ||q|| ||d|| (||s c|| <= ||d|| + e, e <= s sqrt(dim) / 2 <= 0.126 ||d||
//     for dim <= 1024, |t| <= 1): eight of them are < 2^-19;
//   * the stored f32 norms against the true ones, and the bound t itself being a score of the EXACT pass, whose f32 dot product
//     over dim terms is off the true one by at most dim 2^-24 ||q|| ||d||.
//   kappa = dim 2^-24 + 2^-18  (384: 2.7e-5; the mean eps on Gaussian rows is 0.017).
// With c^ = s_q s (c_q.c) / (||q|| ||d||) and eps = B / (||q|| ||d||) + kappa the exact pass's score lies in [c^ - eps, c^ + eps].
//   * KIND 1, the sample: the maximum of c^ - eps over each sampled unit of tiles (the plan of the bf16 filter); the k-th largest
//     of a query's maxima is a score at least k documents reach: the bound t (sample_bound_*, nothing taken off).
//   * KIND 0, the list: every (query, document) with c^ + eps >= t goes to the list of the wave that found it;
//     cosine_rescore_kernel computes those pairs' exact cosines from the F32 rows, topk_candidates_kernel selects: the scores and
//     the order of launch_cosine_search's filter route, bit for bit.
// What the rule cannot judge -- a row with a non-finite value, a norm below 1e-4, s = 0 -- carries ok = 0 in its plane entry and
// PASSES; a query of that kind raises the overflow word itself, and launch_cosine_search answers the call.
//
// Filter kernel.  v_mfma_i32_16x16x64_i8: lane (n = lane % 16, g = lane / 16) gives 16 consecutive code bytes of document n as B
// (the four lanes of a document read 64 contiguous bytes per K-step, one 16-byte load each) and of query n as A; accumulator
// register r of that lane is query 4 g + r x document n.  A wave owns a tile of 16 documents: all NK = dim / 64 loads of the tile
// go out first (NK x 4 VGPRs: 24 at dim 384, 64 at 1 024 -- the whole tile fits the registers at every width, so no pieces),
// the next tile's are requested when this one's MFMAs have consumed them, before its scores are looked at.  No LDS staging of the
// corpus, no barrier in the loop.  The query codes sit in LDS as ready fragments, in QB = 1 / 2 / 4 blocks of 16 queries: one
// query costs one MFMA per K-step, not four.
#include <algorithm>
#include <vector>

#include "device_utils.h"
#include "dynamic_lds.h"
#include "kernels.h"

namespace kjarni {

namespace {

typedef int ci32x4 __attribute__((ext_vector_type(4)));

constexpr int CODED_LIST = 0, CODED_SAMPLE_MAX = 1;
constexpr float kRoundUp = 1.0f + 0x1p-17f;   // e: the f32 sum of dim squares and its root are within 2^-18 of the true norm

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------------------
// Encode: one wave per row (the row in registers: lane l holds the 16-byte pieces l, l + 64, ...), three wave reductions.
//   s     = max|x_i| / 127                    (IEEE division; a NaN element is dropped by the max and caught by the norm)
//   c_i   = rint(x_i / s), 0 where that is not finite
//   ||x|| = per 16-byte piece an fma chain from zero, pieces added in order, xor butterfly over the wave, sqrtf: the one-query
//           streaming scan's arithmetic
//   e     = sqrt(sum (x_i - s c_i)^2) (1 + 2^-17): at least ||r||
//   ok    = 1 if the rule covers the row (s > 0, everything finite, 1e-4 <= ||x|| < inf), else 0
// meta[row] = {s, e, ||x||, ok}.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cosine_encode_kernel(const float* __restrict__ rows, int64_t n_rows, int dim,
                                                            int8_t* __restrict__ codes, f32x4* __restrict__ meta)
{
    const int lane = threadIdx.x & 63, nv4 = dim >> 2;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_rows; row += n_waves) {
        const float* src = rows + row * dim;
        f32x4 x[4];
        float mx = 0.0f, n2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c4 = lane + 64 * i;
            x[i] = c4 < nv4 ? __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + 4 * c4)) : f32x4{0.f, 0.f, 0.f, 0.f};
            float s2 = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                mx = fmaxf(mx, fabsf(x[i][c]));
                s2 = fmaf(x[i][c], x[i][c], s2);
            }
            n2 += s2;
        }
        mx = wave_max(mx);
        const float dn = sqrtf(wave_sum(n2));
        const float s = mx / 127.0f;
        float r2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c4 = lane + 64 * i;
            uint32_t packed = 0u;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float qv = x[i][c] / s;
                const float cf = fabsf(qv) <= 127.5f ? rintf(qv) : 0.0f;   // (NaN, inf, 0 / 0: code 0)
                const float r = fmaf(-s, cf, x[i][c]);
                r2 = fmaf(r, r, r2);
                packed |= ((uint32_t)(int)cf & 0xFFu) << (8 * c);
            }
            if (c4 < nv4) *reinterpret_cast<uint32_t*>(codes + row * dim + 4 * c4) = packed;
        }
        const float e = sqrtf(wave_sum(r2)) * kRoundUp;
        const bool ok = s > 0.0f && s < INFINITY && e < INFINITY && dn >= 1e-4f && dn < INFINITY;
        if (lane == 0) meta[row] = f32x4{s, e, dn, ok ? 1.0f : 0.0f};
    }
}

__global__ void coded_init_kernel(unsigned long long* stats)
{
    if (threadIdx.x < 2) stats[threadIdx.x] = 0ull;
}

struct CodedOut {
    uint64_t* wave_list;    // CODED_LIST: [waves, cap_w] entries (query of the whole call << 32 | document)
    unsigned* wave_count;   // [waves]
    unsigned cap_w;
    unsigned* overflow;     // raised when a list is full
    unsigned long long* passed;   // all waves' entries, summed over the call's launches
    int q_base;
    float* maxima;          // CODED_SAMPLE_MAX: [nq, max_stride]
    int64_t max_stride;
    int64_t units;          // sample units: unit u = unit_tiles consecutive tiles of 16 documents from tile u * tile_stride on
    int tile_stride, unit_tiles;
};

template <int NK, int KIND, int QB>   // dim = 64 NK, up to 16 QB queries
__global__ __launch_bounds__(256, 2) void cosine_filter_i8_kernel(const int8_t* __restrict__ qcodes, const f32x4* __restrict__ qmeta, int nq,
                                                                  const int8_t* __restrict__ codes, const f32x4* __restrict__ meta,
                                                                  int64_t n_docs, const float* __restrict__ thr_score,
                                                                  const int64_t* __restrict__ thr_idx, float kappa, CodedOut out)
{
    constexpr int dim = 64 * NK, NQ = 16 * QB;
    extern __shared__ __attribute__((aligned(16))) uint8_t csm[];
    ci32x4* sQf = reinterpret_cast<ci32x4*>(csm);                      // [NK][QB][64 lanes]: A fragments, ready to use
    f32x4* sPar = reinterpret_cast<f32x4*>(csm + NK * QB * 1024);      // [4 groups][QB][4]: the lane groups' query parameters
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, g = lane >> 4;
    for (int f = tid; f < NK * QB * 64; f += 256) {
        const int l = f & 63, b = (f >> 6) % QB, s = (f >> 6) / QB;
        const int q = 16 * b + (l & 15);
        ci32x4 v = {0, 0, 0, 0};
        if (q < nq) v = *reinterpret_cast<const ci32x4*>(qcodes + (int64_t)q * dim + 64 * s + 16 * (l >> 4));
        sQf[f] = v;
    }
    // Per query, with a_q = (||q|| + e_q) and b_q = e_q (both rounded up by the slack's share):
    //   list:    pass  <=>  s_q (s I) + a_q e + w_q ||d|| >= 0,   w_q = e_q + (kappa - t) ||q||     -> {s_q, a_q, w_q, -}
    //            a row past nq: w = -inf (nothing passes); no bound / a query the rule does not cover: s = a = 0, w = +inf
    //   sample:  c^ - eps = (s_q (s I) - a_q e) / (||q|| ||d||) - c_q,   c_q = e_q / ||q|| + kappa   -> {s_q, a_q, 1 / ||q||, c_q}
    //            a query the rule does not cover or a row past nq: 1 / ||q|| = NaN (its maxima come out as "no bound")
    if (tid < NQ) {
        f32x4 p;
        const bool real = tid < nq;
        const f32x4 m = real ? qmeta[tid] : f32x4{0.f, 0.f, 0.f, 0.f};
        const float qn = m[2], aq = (qn + m[1]) * kRoundUp;
        if (KIND == CODED_SAMPLE_MAX) {
            p = f32x4{m[0], aq, (real && m[3] != 0.0f) ? 1.0f / qn : __builtin_nanf(""), (m[1] / qn) * kRoundUp + kappa};
        } else {
            float t = -INFINITY;
            if (real && thr_idx[tid] >= 0) t = thr_score[tid];
            const float w = m[1] * kRoundUp + (kappa - t) * qn;
            if (!real) p = f32x4{0.f, 0.f, -INFINITY, 0.f};
            else if (t == -INFINITY || m[3] == 0.0f || w != w) {
                p = f32x4{0.f, 0.f, INFINITY, 0.f};
                *out.overflow = 1u;   // (every pair of this query would pass: launch_cosine_search answers the call)
            } else p = f32x4{m[0], aq, w, 0.f};
        }
        // query 16 b + 4 g + r -> slot (g, b, r)
        const int b = tid >> 4, gg = (tid & 15) >> 2, r = tid & 3;
        sPar[(gg * QB + b) * 4 + r] = p;
    }
    __syncthreads();
    uint32_t realq = 0u;   // bit 4 b + r: this lane's query (b, r) exists
#pragma unroll
    for (int e = 0; e < 4 * QB; ++e) realq |= (16 * (e >> 2) + 4 * g + (e & 3)) < nq ? 1u << e : 0u;

    const int64_t all_tiles = (n_docs + 15) >> 4;
    const int64_t waves = (int64_t)gridDim.x * 4, wave = (int64_t)blockIdx.x * 4 + wid;
    const uint32_t voff = (uint32_t)(n16 * dim + 16 * g);
    // a tile's 16 rows of codes and its plane entries requested (past the corpus: descriptors without extent -- zeros, no traffic)
    auto request = [&](int64_t tile, ci32x4 (&x)[NK], f32x4& md) {
        const int64_t d0 = tile << 4;
        int64_t rows = n_docs - d0 < 16 ? n_docs - d0 : 16;
        rows = rows > 0 ? rows : 0;
        const int64_t base = rows > 0 ? d0 : 0;
        const __amdgpu_buffer_rsrc_t rC =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t*>(codes + base * dim), 0, (int)(rows * dim), 0x00020000);
        const __amdgpu_buffer_rsrc_t rM =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<f32x4*>(meta + base), 0, (int)(rows * 16), 0x00020000);
#pragma unroll
        for (int s = 0; s < NK; ++s) x[s] = __builtin_bit_cast(ci32x4, __builtin_amdgcn_raw_buffer_load_b128(rC, voff + 64 * s, 0, 0));
        md = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rM, (uint32_t)(16 * n16), 0, 0));
    };
    // the tile's integer dot products; `next`'s rows are requested as soon as the MFMAs have taken this tile's
    auto tile_dots = [&](int64_t next, ci32x4 (&x)[NK], f32x4& mnext, ci32x4 (&acc)[QB]) {
        // (the query fragments and parameters are read from LDS here, every tile: hoisted out of the tile loop they are up to
        // 4 NK QB + 16 QB live registers)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int b = 0; b < QB; ++b) acc[b] = ci32x4{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < NK; ++s)
#pragma unroll
            for (int b = 0; b < QB; ++b) acc[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(sQf[(s * QB + b) * 64 + lane], x[s], acc[b], 0, 0, 0);
        request(next, x, mnext);
    };
    ci32x4 x[NK];
    f32x4 mnext;
    if constexpr (KIND == CODED_SAMPLE_MAX) {
        request(wave < out.units ? wave * out.tile_stride : all_tiles, x, mnext);
        for (int64_t it = wave; it < out.units; it += waves) {
            float run[4 * QB];
#pragma unroll
            for (int e = 0; e < 4 * QB; ++e) run[e] = -INFINITY;
#pragma unroll 1
            for (int u = 0; u < out.unit_tiles; ++u) {
                const int64_t tile = it * out.tile_stride + u;
                const int64_t next = u + 1 < out.unit_tiles ? tile + 1 : (it + waves < out.units ? (it + waves) * out.tile_stride : all_tiles);
                const f32x4 md = mnext;
                ci32x4 acc[QB];
                tile_dots(next, x, mnext, acc);
                const bool ok = (tile << 4) + n16 < n_docs && md[3] != 0.0f;
                const float idn = __builtin_amdgcn_rcpf(md[2]);
#pragma unroll
                for (int e = 0; e < 4 * QB; ++e) {
                    const f32x4 p = sPar[(g * QB + (e >> 2)) * 4 + (e & 3)];
                    const float num = fmaf(p[0], md[0] * (float)acc[e >> 2][e & 3], -(p[1] * md[1]));
                    run[e] = fmaxf(run[e], ok ? fmaf(num, idn * p[2], -p[3]) : -INFINITY);   // (a NaN -- no bound -- is dropped)
                }
            }
#pragma unroll
            for (int e = 0; e < 4 * QB; ++e) {
                const float m = row16_max_desc(run[e]);
                const int q = 16 * (e >> 2) + 4 * g + (e & 3);
                if (n16 == 0 && q < nq) out.maxima[(int64_t)q * out.max_stride + it] = m;
            }
        }
        return;
    }
    unsigned count = 0;   // entries in this wave's list (wave-uniform)
    request(wave, x, mnext);
    for (int64_t it = wave; it < all_tiles; it += waves) {
        const f32x4 md = mnext;
        ci32x4 acc[QB];
        tile_dots(it + waves, x, mnext, acc);
        const int64_t ad = (it << 4) + n16;
        const bool odd_doc = md[3] == 0.0f;
        uint32_t mask = 0u;
#pragma unroll
        for (int e = 0; e < 4 * QB; ++e) {
            const f32x4 p = sPar[(g * QB + (e >> 2)) * 4 + (e & 3)];
            const float margin = fmaf(p[0], md[0] * (float)acc[e >> 2][e & 3], fmaf(p[1], md[1], p[2] * md[2]));
            mask |= (odd_doc || !(margin < 0.0f)) ? 1u << e : 0u;   // (a NaN margin passes)
        }
        mask &= realq;
        if (ad >= n_docs) mask = 0u;
        uint64_t lanes = __ballot(mask != 0u);
        if (lanes == 0ull) continue;
        const unsigned mine = (unsigned)__popc(mask);
#pragma nounroll
        while (lanes != 0ull) {
            const int leader = __ffsll((long long)lanes) - 1;
            const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)mine, leader);
            if (lane == leader) {
                unsigned at = count;
#pragma nounroll
                for (uint32_t mm = mask; mm != 0u; mm &= mm - 1u, ++at) {
                    const int e = __ffs((int)mm) - 1;
                    const int q = out.q_base + 16 * (e >> 2) + 4 * g + (e & 3);
                    if (at < out.cap_w) out.wave_list[(size_t)wave * out.cap_w + at] = ((uint64_t)(uint32_t)q << 32) | (uint64_t)(uint32_t)ad;
                    else *out.overflow = 1u;   // launch_cosine_search answers instead
                }
            }
            count += c;
            lanes &= lanes - 1ull;
        }
    }
    if (lane == 0) {
        out.wave_count[wave] = count < out.cap_w ? count : out.cap_w;
        if (count != 0u) atomicAdd(out.passed, (unsigned long long)count);
    }
}

// The passes' shape.  Sample: the bf16 filter's plan (about a twentieth of a large corpus, an eighth of a small one, at most
// 4 096 units).  Lists: sized from the corpus and the grid -- room for one pair in 16 of a query block's, between 2^16 and 2^22
// entries over all waves, dealt evenly to the grid's waves (Gaussian rows at dim 384, k = 10 pass one pair in 120 at 50 001
// documents, fewer the larger the sample; a wave's share varies around the mean).
struct CodedPlan {
    int nk;
    int64_t units;
    int tile_stride, unit_tiles;
    size_t list_entries;
};
CodedPlan coded_plan(int64_t n_docs, int dim, int nq)
{
    CodedPlan p{};
    p.nk = dim / 64;
    const int64_t tiles = (n_docs + 15) / 16;
    p.unit_tiles = (int)std::min<int64_t>(16, std::max<int64_t>(1, (tiles + 4096 * 20 - 1) / (4096 * 20)));
    p.units = std::min<int64_t>(4096, std::max<int64_t>(1, tiles / p.unit_tiles / 8));
    p.tile_stride = (int)std::max<int64_t>(p.unit_tiles, tiles / p.units);
    const int64_t pairs = n_docs * std::min(nq, 64);
    p.list_entries = (size_t)std::min<int64_t>((int64_t)1 << 22, std::max<int64_t>((int64_t)1 << 16, pairs / 16));
    return p;
}
inline int coded_qb(int m) { return m <= 16 ? 1 : (m <= 32 ? 2 : 4); }
// workgroups: four per CU for one block of queries (its waves hold a tile and 4 accumulators), two otherwise
inline unsigned coded_grid(int64_t n_docs, int qb)
{
    const int64_t tiles = (n_docs + 15) / 16;
    return (unsigned)std::min<int64_t>((tiles + 3) / 4, 256 * (qb == 1 ? 4 : 2));
}

template <int KIND>
hipError_t coded_launch(int nk, unsigned grid, const int8_t* qcodes, const f32x4* qmeta, int m, const int8_t* codes, const f32x4* meta,
                        int64_t n_docs, const float* thr_score, const int64_t* thr_idx, float kappa, const CodedOut& out, hipStream_t stream)
{
    const int qb = coded_qb(m);
    const size_t lds = (size_t)nk * qb * 1024 + (size_t)16 * qb * 16;
#define KJ_CODED(NK_, QB_)                                                                                                       \
    do {                                                                                                                         \
        auto kern = cosine_filter_i8_kernel<NK_, KIND, QB_>;                                                                     \
        if (lds > 48 * 1024) {                                                                                                   \
            const hipError_t ea = allow_dynamic_lds(kern, lds);                                                                  \
            if (ea != hipSuccess) return ea;                                                                                     \
        }                                                                                                                        \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, stream, qcodes, qmeta, m, codes, meta, n_docs, thr_score, thr_idx, kappa, out); \
    } while (0)
#define KJ_CODED_Q(NK_)                                                                                                          \
    do {                                                                                                                         \
        if (qb == 1) KJ_CODED(NK_, 1);                                                                                           \
        else if (qb == 2) KJ_CODED(NK_, 2);                                                                                      \
        else KJ_CODED(NK_, 4);                                                                                                   \
    } while (0)
    switch (nk) {
    case 2: KJ_CODED_Q(2); break;
    case 4: KJ_CODED_Q(4); break;
    case 6: KJ_CODED_Q(6); break;
    case 8: KJ_CODED_Q(8); break;
    case 12: KJ_CODED_Q(12); break;
    case 16: KJ_CODED_Q(16); break;
    default: return hipErrorInvalidValue;
    }
#undef KJ_CODED_Q
#undef KJ_CODED
    return hipGetLastError();
}

// workspace layout of the coded route (behind launch_cosine_search's own workspace, which the fallback uses)
struct CodedWs {
    int8_t* qcodes;
    f32x4* qmeta;
    float* qn2;
    float* maxima;
    float* thr_score;
    int64_t* thr_idx;
    unsigned* counters;
    uint64_t* wave_list;
    unsigned* wave_count;
    uint64_t* cand_key;
    unsigned long long* stats;
    unsigned cap_q;
    size_t counter_bytes, bytes;
};
CodedWs coded_ws(uint8_t* base, int nq, int dim, const CodedPlan& p)
{
    CodedWs w{};
    uint8_t* at = base;
    auto take = [&](size_t b) {
        uint8_t* r = at;
        at += pad256(b);
        return r;
    };
    w.qcodes = reinterpret_cast<int8_t*>(take((size_t)nq * dim));
    w.qmeta = reinterpret_cast<f32x4*>(take((size_t)nq * 16));
    w.qn2 = reinterpret_cast<float*>(take((size_t)(nq + 8) * 4));
    w.maxima = reinterpret_cast<float*>(take((size_t)nq * 4096 * 4));
    w.thr_score = reinterpret_cast<float*>(take((size_t)nq * 4));
    w.thr_idx = reinterpret_cast<int64_t*>(take((size_t)nq * 8));
    w.counter_bytes = (size_t)(nq + 1) * cosine_count_stride() * 4;
    w.counters = reinterpret_cast<unsigned*>(take(w.counter_bytes));
    w.wave_list = reinterpret_cast<uint64_t*>(take(p.list_entries * 8));
    w.wave_count = reinterpret_cast<unsigned*>(take(4096 * 4));
    w.cap_q = (unsigned)std::min<size_t>(65536, ((size_t)4 << 20) / (size_t)nq);   // candidates per query after rescoring
    w.cand_key = reinterpret_cast<uint64_t*>(take((size_t)w.cap_q * nq * 8));
    w.stats = reinterpret_cast<unsigned long long*>(take(16));
    w.bytes = (size_t)(at - base);
    return w;
}

}  // namespace

size_t cosine_codes_bytes(int64_t n_docs, int dim) { return pad256((size_t)n_docs * dim) + (size_t)n_docs * 16; }

hipError_t launch_cosine_encode(const float* rows, int64_t n_rows, int dim, int8_t* codes, float* meta, hipStream_t stream)
{
    if (n_rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 256 * 8);
    hipLaunchKernelGGL(cosine_encode_kernel, dim3(grid), dim3(256), 0, stream, rows, n_rows, dim, codes, reinterpret_cast<f32x4*>(meta));
    return hipGetLastError();
}

hipError_t launch_cosine_encode_plane(const float* corpus, int64_t n_docs, int dim, void* plane, hipStream_t stream)
{
    int8_t* codes = static_cast<int8_t*>(plane);
    return launch_cosine_encode(corpus, n_docs, dim, codes, reinterpret_cast<float*>(codes + pad256((size_t)n_docs * dim)), stream);
}

// The shapes the int8 passes answer themselves; everything else the call hands to launch_cosine_search (stats[3] = 2).
bool cosine_coded_serves(int nq, int64_t n_docs, int dim, int k)
{
    if (!cosine_filter_width(dim) || n_docs < 20000 || n_docs >= (int64_t)0xFFFFFFFF || nq < 1 || nq > 1024 || k < 1) return false;
    return coded_plan(n_docs, dim, nq).units >= 8 * (int64_t)k;   // (the sample bounds k: as for the bf16 sample)
}

size_t cosine_search_coded_workspace_bytes(int nq, int64_t n_docs, int dim, int k, bool one_query_aligned)
{
    const size_t own = one_query_aligned ? cosine_search_one_query_workspace_bytes(n_docs, dim, k) : cosine_search_workspace_bytes(nq, n_docs, dim, k);
    if (!cosine_coded_serves(nq, n_docs, dim, k)) return pad256(own);
    return pad256(own) + coded_ws(nullptr, nq, dim, coded_plan(n_docs, dim, nq)).bytes;
}

// stats (host, optional): pairs judged, pairs passed, candidates after rescoring, fallback (0: the int8 route answered; 1: a list
// overflowed and launch_cosine_search answered; 2: a shape the route does not serve, launch_cosine_search answered).
// Waits for the stream: the overflow word decides on the host which search's results stand.
hipError_t launch_cosine_search_coded(const float* queries, int nq, const float* corpus, int64_t n_docs, int dim, int mode, int k,
                                      const void* plane, void* workspace, bool one_query_aligned, int64_t* out_idx, float* out_score,
                                      uint64_t* stats, hipStream_t stream)
{
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (nq <= 0 || k <= 0) return hipSuccess;
    if (n_docs <= 0 || n_docs >= (int64_t)0xFFFFFFFF) return hipErrorInvalidValue;
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(corpus) | reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(plane)) & 15) == 0;
    if (!cosine_coded_serves(nq, n_docs, dim, k) || !aligned16 || (mode != 0 && mode != 1)) {
        if (stats) stats[3] = 2;
        return launch_cosine_search(queries, nq, corpus, n_docs, dim, mode, k, workspace, out_idx, out_score, stream);
    }
    const size_t own = one_query_aligned ? cosine_search_one_query_workspace_bytes(n_docs, dim, k) : cosine_search_workspace_bytes(nq, n_docs, dim, k);
    const CodedPlan p = coded_plan(n_docs, dim, nq);
    const CodedWs w = coded_ws(static_cast<uint8_t*>(workspace) + pad256(own), nq, dim, p);
    const int8_t* codes = static_cast<const int8_t*>(plane);
    const f32x4* meta = reinterpret_cast<const f32x4*>(codes + pad256((size_t)n_docs * dim));
    const float kappa = (float)dim * 0x1p-24f + 0x1p-18f;

    hipLaunchKernelGGL(coded_init_kernel, dim3(1), dim3(64), 0, stream, w.stats);
    hipError_t e = launch_cosine_encode(queries, nq, dim, w.qcodes, reinterpret_cast<float*>(w.qmeta), stream);
    if (e != hipSuccess) return e;
    e = cosine_query_sqnorms(queries, nq, dim, w.qn2, stream);
    if (e != hipSuccess) return e;
    for (int q0 = 0; q0 < nq; q0 += 64) {
        const int m = std::min(64, nq - q0);
        CodedOut out{};
        out.maxima = w.maxima + (int64_t)q0 * p.units;
        out.max_stride = p.units;
        out.units = p.units;
        out.tile_stride = p.tile_stride;
        out.unit_tiles = p.unit_tiles;
        const unsigned grid = (unsigned)std::min<int64_t>((p.units + 3) / 4, 512);
        e = coded_launch<CODED_SAMPLE_MAX>(p.nk, grid, w.qcodes + (int64_t)q0 * dim, w.qmeta + q0, m, codes, meta, n_docs, nullptr, nullptr, kappa,
                                           out, stream);
        if (e != hipSuccess) return e;
    }
    // the bounds (nothing taken off: the maxima are lower bounds already); zeroes the candidate counters
    e = cosine_sample_bound(w.maxima, (int)p.units, nq, k, w.thr_score, w.thr_idx, w.counters, stream);
    if (e != hipSuccess) return e;
    for (int q0 = 0; q0 < nq; q0 += 64) {
        const int m = std::min(64, nq - q0);
        const unsigned grid = coded_grid(n_docs, coded_qb(m));
        CodedOut out{};
        out.wave_list = w.wave_list;
        out.wave_count = w.wave_count;
        out.cap_w = (unsigned)(p.list_entries / ((size_t)grid * 4));
        out.overflow = w.counters;
        out.passed = w.stats;
        out.q_base = q0;
        e = coded_launch<CODED_LIST>(p.nk, grid, w.qcodes + (int64_t)q0 * dim, w.qmeta + q0, m, codes, meta, n_docs, w.thr_score + q0,
                                     w.thr_idx + q0, kappa, out, stream);
        if (e != hipSuccess) return e;
        // the exact cosines of what passed, from the f32 rows (queries, bounds and lists of the WHOLE call)
        e = cosine_rescore(mode, dim, queries, corpus, w.qn2, w.thr_score, w.thr_idx, w.wave_list, w.wave_count, (int)grid * 4, out.cap_w,
                           w.counters, w.cap_q, w.cand_key, stream);
        if (e != hipSuccess) return e;
    }
    e = cosine_topk_candidates(k, nq, w.cand_key, w.counters, w.cap_q, out_idx, out_score, stream);
    if (e != hipSuccess) return e;
    std::vector<unsigned> counters(w.counter_bytes / 4);
    unsigned long long passed[2] = {0, 0};
    e = hipMemcpyAsync(counters.data(), w.counters, w.counter_bytes, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(passed, w.stats, 16, hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) return e;
    e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    const bool overflow = counters[0] != 0u;
    if (stats) {
        stats[0] = (uint64_t)nq * (uint64_t)n_docs;
        stats[1] = passed[0];
        for (int q = 0; q < nq; ++q) stats[2] += counters[(size_t)cosine_count_stride() * (1 + q)];
        stats[3] = overflow ? 1 : 0;
    }
    if (!overflow) return hipSuccess;
    return launch_cosine_search(queries, nq, corpus, n_docs, dim, mode, k, workspace, out_idx, out_score, stream);
}

}  // namespace kjarni
