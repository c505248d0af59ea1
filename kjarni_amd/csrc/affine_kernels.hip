// GGUF Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K matrices resident in HBM (gfx950): the decode projection for <= 8 rows, dequantization
// for the prompt route, embedding gather.
//
// One thing on the device.  Over every run of 32 elements all five types are w = a * q + b, q an unsigned 4- or 5-bit code and
// a, b two f32 numbers:  Q4_0 (d, -8 d)   Q5_0 (d, -16 d)   Q4_1 / Q5_1 (d, m)   Q5_K sub-block j (d * sc_j, -(dmin * m_j)).
// d, dmin, m are f16 (11 significant bits), sc_j, m_j <= 63, q <= 31: every product is exact in f32 and fmaf(a, q, b) rounds once,
// in the add, as ggml_dequantize_row (gguf.cpp) does.  (The one difference: a weight that is exactly zero under a negative d is
// -0.0 there and +0.0 here.)
//
// Device layout "affine-32".  Every matrix [n, k] (k % 32 == 0) is repacked at load into planes, each its own 256-byte aligned
// allocation, rows in HF order, runs of a row contiguous:
//   q   u8  [n, k / 2]        16 bytes per run: byte i holds element i (low nibble) and element i + 16 (high nibble) -- the 32-block
//                             types' own order; a Q5_K sub-block is re-nibbled into it
//   q2  u32 [n, k / 32]       5-bit types: bit e of the word is element e's fifth bit
//   s   f32 [n, k / 32, 2]    (a, b) of the run, formed on the host with the f32 operations above
// Q8_0 is the same family with signed 8-bit codes and b = 0; the projection reads it from the planes quant_kernels.hip describes.
//
// Decode projection (affine_proj_kernel).  A workgroup of 4 waves stages the activation rows in LDS once per K chunk of 1 024
// elements (32 runs; 8 rows are 36 KB), RMS-normalised where the stage has a norm, with the sum of every (row, run) beside them.
// A wave is split over (column, run): lane l works on run l % 32 of the chunk for column l / 32 of each of its P column pairs, so at
// K = 896 (28 runs) 56 of 64 lanes carry weight bytes.  Per run a lane loads 16 bytes of nibbles (+ 4 of fifth bits, + 8 of
// (a, b)), turns the codes into f32 integers (mask + v_cvt_f32_ubyte; the fifth bits of four elements are spread to their
// bytes by one multiply) and accumulates raw code x activation sums for every row; the scales enter once per run:
//   dot += a * sum(q x) + b * sum(x).
// The activations of a run come from LDS as 16-byte reads shared by the lane's P columns; runs are 36 floats apart so the 16 lanes
// of a read phase hit 64 different banks.  A half-wave reduction (fixed order: the same bits on every call) and the stage's
// epilogue (bias, cache-row offset, SwiGLU, residual) finish the columns.  No atomics, no scratch.
#include "affine_kernels.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "gguf.h"

namespace kjarni {

namespace {

constexpr int kChunk = 1024;             // elements of a row staged at a time
constexpr int kRunStride = 36;           // floats between the runs of a staged row (32 + 4: conflict-free 16-byte reads)
constexpr int kRowStride = 32 * kRunStride;

__host__ __device__ inline int code_bits(uint32_t type)
{
    return type == GGML_Q8_0 ? 8 : ((type == GGML_Q4_0 || type == GGML_Q4_1) ? 4 : ((type == GGML_Q5_0 || type == GGML_Q5_1 || type == GGML_Q5_K) ? 5 : 0));
}

// One column of one matrix as a lane reads it: the row starts of its planes.
struct Col {
    const uint8_t* q;
    const uint32_t* h;
    const float* s;
    int bits;  // 0: no column (past the end)
};

__device__ inline Col column_of(const QMat& W, int c, int k)
{
    Col o;
    o.bits = code_bits(W.type);
    const int64_t runs = k / 32;
    if (o.bits == 8) {
        o.q = static_cast<const uint8_t*>(W.q) + (int64_t)c * k;
        o.h = nullptr;
        o.s = static_cast<const float*>(W.s) + c * runs;
    } else {
        o.q = static_cast<const uint8_t*>(W.q) + (int64_t)c * (k / 2);
        o.h = static_cast<const uint32_t*>(W.q2) + c * runs;
        o.s = static_cast<const float*>(W.s) + c * runs * 2;
    }
    return o;
}

// The codes of one run in registers, and its (a, b).
struct Run {
    uint32_t lo[4], hi[4];  // 4 / 5 bits: lo = the 16 nibble bytes; 8 bits: lo / hi = the 32 code bytes
    uint32_t h;
    float a, b;
};

template <int BITS>
__device__ inline void load_run(const Col& c, int run, Run& o)
{
    if constexpr (BITS == 8) {
        const uint4* p = reinterpret_cast<const uint4*>(c.q + (int64_t)run * 32);
        const uint4 v0 = p[0], v1 = p[1];
        o.lo[0] = v0.x; o.lo[1] = v0.y; o.lo[2] = v0.z; o.lo[3] = v0.w;
        o.hi[0] = v1.x; o.hi[1] = v1.y; o.hi[2] = v1.z; o.hi[3] = v1.w;
        o.a = c.s[run];
        o.b = 0.0f;
    } else {
        const uint4 v0 = *reinterpret_cast<const uint4*>(c.q + (int64_t)run * 16);
        o.lo[0] = v0.x; o.lo[1] = v0.y; o.lo[2] = v0.z; o.lo[3] = v0.w;
        if constexpr (BITS == 5) o.h = c.h[run];
        const float2 ab = *reinterpret_cast<const float2*>(c.s + 2 * (int64_t)run);
        o.a = ab.x;
        o.b = ab.y;
    }
}

// bits 0..3 of x to bit 4 of bytes 0..3 (the four shifted copies of the multiply do not overlap)
__device__ inline uint32_t spread_fifth(uint32_t x) { return (((x & 0xFu) * 0x00204081u) & 0x01010101u) << 4; }

// Word w (0..3, a constant after unrolling) of a run: elements 4w .. 4w + 3 into f[0..3], 16 + 4w .. 16 + 4w + 3 into f[4..7].
template <int BITS>
__device__ inline void unpack(const Run& r, int w, float (&f)[8])
{
    if constexpr (BITS == 8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[i] = (float)(int8_t)(r.lo[w] >> (8 * i));
            f[4 + i] = (float)(int8_t)(r.hi[w] >> (8 * i));
        }
    } else {
        uint32_t l = r.lo[w] & 0x0F0F0F0Fu, u = (r.lo[w] >> 4) & 0x0F0F0F0Fu;
        if constexpr (BITS == 5) {
            l |= spread_fifth(r.h >> (4 * w));
            u |= spread_fifth(r.h >> (16 + 4 * w));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[i] = (float)((l >> (8 * i)) & 0xFFu);
            f[4 + i] = (float)((u >> (8 * i)) & 0xFFu);
        }
    }
}

// One staged chunk for the lane's P columns, all of width BITS: raw code x activation sums per row, then the run's (a, b) once.
template <int BITS, int R, int P>
__device__ inline void chunk_columns(const Col (&col)[P], int run, int runs, int rl, const float (*xs)[kRowStride], const float (*rs)[32],
                                     float (&acc)[P][R])
{
    Run rn[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rn[p].lo[i] = rn[p].hi[i] = 0u;
        rn[p].h = 0u;
        rn[p].a = rn[p].b = 0.0f;
        if (run < runs && col[p].bits != 0) load_run<BITS>(col[p], run, rn[p]);
    }
    float dq[P][R];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) dq[p][r] = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float f[P][8];
#pragma unroll
        for (int p = 0; p < P; ++p) unpack<BITS>(rn[p], w, f[p]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float4 x0 = *reinterpret_cast<const float4*>(&xs[r][rl * kRunStride + 4 * w]);
            const float4 x1 = *reinterpret_cast<const float4*>(&xs[r][rl * kRunStride + 16 + 4 * w]);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float d = dq[p][r];
                d = fmaf(f[p][0], x0.x, d); d = fmaf(f[p][1], x0.y, d); d = fmaf(f[p][2], x0.z, d); d = fmaf(f[p][3], x0.w, d);
                d = fmaf(f[p][4], x1.x, d); d = fmaf(f[p][5], x1.y, d); d = fmaf(f[p][6], x1.z, d); d = fmaf(f[p][7], x1.w, d);
                dq[p][r] = d;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float sx = rs[r][rl];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p][r] = fmaf(rn[p].a, dq[p][r], fmaf(rn[p].b, sx, acc[p][r]));
    }
}

// TC: the code width of every column of the launch (4, 5, 8), or 0: each column's own (P = 1; wave-uniform but for a pair that
// straddles two segments, or gate / up of different widths -- the half-waves then take their turns).
// 256 threads = 4 waves; a wave takes P column pairs (SwiGLU: P columns, gate in lanes 0..31 and up in lanes 32..63).
template <int TC, int R, int P>
__global__ __launch_bounds__(256) void affine_proj_kernel(AffineProjArgs a, int k)
{
    __shared__ __attribute__((aligned(16))) float xs[R][kRowStride];
    __shared__ float rs[R][32];
    __shared__ float inv[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, rl = lane & 31;
    const int runs = k / 32;
    if (a.gamma) {  // 1 / rms of every row, one wave per row
        for (int r = wave; r < a.rows; r += 4) {
            const float* row = a.X + r * a.ldx;
            float s = 0.0f;
            for (int i = lane * 4; i < k; i += 256) {
                const float4 v = *reinterpret_cast<const float4*>(row + i);
                s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) inv[r] = 1.0f / sqrtf(s / (float)k + a.eps);
        }
    }
    // the lane's columns: segment, column inside it, plane rows
    const int n0 = a.W[0].n, n1 = a.mode == AF_QKV ? a.W[1].n : 0, n2 = a.mode == AF_QKV ? a.W[2].n : 0;
    Col col[P];
    int seg[P], cin[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int slot = (blockIdx.x * 4 + wave) * P + p;
        col[p].bits = 0; col[p].q = nullptr; col[p].h = nullptr; col[p].s = nullptr;
        seg[p] = 0;
        if (a.mode == AF_SWIGLU) {
            cin[p] = slot;
            seg[p] = half;
            if (slot < n0) col[p] = half == 0 ? column_of(a.W[0], slot, k) : column_of(a.W[1], slot, k);
        } else {
            int g = 2 * slot + half;
            if (g >= n0) {
                g -= n0;
                seg[p] = 1;
                if (g >= n1) {
                    g -= n1;
                    seg[p] = 2;
                }
            }
            cin[p] = g;
            // (selected by value: a runtime index into the argument arrays would put them in scratch)
            if (seg[p] == 0) col[p] = column_of(a.W[0], g, k);
            else if (seg[p] == 1) col[p] = column_of(a.W[1], g, k);
            else if (g < n2) col[p] = column_of(a.W[2], g, k);
        }
    }
    float acc[P][R];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[p][r] = 0.0f;

    for (int c0 = 0; c0 < k; c0 += kChunk) {
        __syncthreads();  // the chunk before is consumed (first pass: inv[] is written)
        {   // stage: thread t holds elements 4t .. 4t + 3 of the chunk; 8 threads make a run
            const int e = c0 + tid * 4;
            float4 g = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (a.gamma && e < k) g = *reinterpret_cast<const float4*>(a.gamma + e);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (r < a.rows && e < k) {
                    v = *reinterpret_cast<const float4*>(a.X + r * a.ldx + e);
                    if (a.gamma) {
                        const float iv = inv[r];
                        v.x = v.x * iv * g.x; v.y = v.y * iv * g.y; v.z = v.z * iv * g.z; v.w = v.w * iv * g.w;
                    }
                }
                *reinterpret_cast<float4*>(&xs[r][(tid >> 3) * kRunStride + (tid & 7) * 4]) = v;
                float t = (v.x + v.y) + (v.z + v.w);
                t += __shfl_xor(t, 1, 64);
                t += __shfl_xor(t, 2, 64);
                t += __shfl_xor(t, 4, 64);
                if ((tid & 7) == 0) rs[r][tid >> 3] = t;
            }
        }
        __syncthreads();
        const int run = c0 / 32 + rl;  // absolute: the planes and the run sums of the chunk are indexed from here
        if constexpr (TC != 0) {
            chunk_columns<TC, R, P>(col, run, runs, rl, xs, rs, acc);
        } else {
            static_assert(TC != 0 || P == 1, "mixed widths: one column pair per wave");
            if (col[0].bits == 4) chunk_columns<4, R, P>(col, run, runs, rl, xs, rs, acc);
            else if (col[0].bits == 5) chunk_columns<5, R, P>(col, run, runs, rl, xs, rs, acc);
            else if (col[0].bits == 8) chunk_columns<8, R, P>(col, run, runs, rl, xs, rs, acc);
        }
    }

    const int off = a.row_off_ptr ? *a.row_off_ptr : a.row_off;
#pragma unroll
    for (int p = 0; p < P; ++p) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = acc[p][r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            const float other = __shfl_xor(v, 32, 64);  // SwiGLU: the up column beside the gate column
            if (r >= a.rows || col[p].bits == 0 || rl != 0) continue;
            const int c = cin[p];
            if (a.mode == AF_SWIGLU) {
                if (half == 0) a.Y[0][(int64_t)r * a.ldy[0] + c] = (v / (1.0f + expf(-v))) * other;
                continue;
            }
            const int s = seg[p];
            if (a.bias) v += a.bias[(s == 0 ? a.bias_off[0] : (s == 1 ? a.bias_off[1] : a.bias_off[2])) + c];
            if (a.R) v += a.R[(int64_t)r * a.ldr + c];
            float* Y = s == 0 ? a.Y[0] : (s == 1 ? a.Y[1] : a.Y[2]);
            const int64_t ldy = s == 0 ? a.ldy[0] : (s == 1 ? a.ldy[1] : a.ldy[2]);
            const int base = (a.mode == AF_QKV && s > 0) ? off : 0;  // K / V rows land at the cache position
            Y[((int64_t)base + r) * ldy + c] = v;
        }
    }
}

// element (row, col) of an affine-32 matrix
__device__ inline float affine_element(const QMat& W, int64_t row, int col)
{
    const int64_t run = row * (W.k / 32) + col / 32;
    const int e = col % 32;
    const uint8_t byte = static_cast<const uint8_t*>(W.q)[run * 16 + (e & 15)];
    uint32_t q = e < 16 ? (byte & 0xFu) : (byte >> 4);
    if (W.q2) q |= ((static_cast<const uint32_t*>(W.q2)[run] >> e) & 1u) << 4;
    const float* ab = static_cast<const float*>(W.s) + 2 * run;
    return fmaf(ab[0], (float)q, ab[1]);
}

// A thread per half-run h: the run's 16 nibble bytes in one load, elements 16 h .. 16 h + 15 out as four 16-byte stores.
__global__ __launch_bounds__(256) void affine_dequant_kernel(QMat W, float* out)
{
    const int64_t halves = (int64_t)W.n * (W.k / 32) * 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < halves; i += (int64_t)gridDim.x * 256) {
        const int64_t run = i >> 1;
        const int h = (int)(i & 1);
        const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(W.q) + run * 16);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t fifth = W.q2 ? static_cast<const uint32_t*>(W.q2)[run] >> (16 * h) : 0u;
        const float2 ab = reinterpret_cast<const float2*>(W.s)[run];
        float4* o = reinterpret_cast<float4*>(out + run * 32 + 16 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = ((w[j] >> (4 * h)) & 0x0F0F0F0Fu) | spread_fifth(fifth >> (4 * j));
            o[j] = make_float4(fmaf(ab.x, (float)(c & 0xFFu), ab.y), fmaf(ab.x, (float)((c >> 8) & 0xFFu), ab.y),
                               fmaf(ab.x, (float)((c >> 16) & 0xFFu), ab.y), fmaf(ab.x, (float)(c >> 24), ab.y));
        }
    }
}

__global__ __launch_bounds__(256) void affine_embed_kernel(const uint32_t* ids, QMat table, float* out)
{
    const uint32_t id = ids[blockIdx.x];
    float* o = out + (int64_t)blockIdx.x * table.k;
    for (int c = threadIdx.x; c < table.k; c += 256) o[c] = id < (uint32_t)table.n ? affine_element(table, id, c) : 0.0f;
}

template <int TC, int R>
void launch_instance(const AffineProjArgs& a, int k, int64_t cols, hipStream_t stream)
{
    // columns per wave: 2 P (SwiGLU: P).  More columns per workgroup spread the staging of the rows over more weight bytes; fewer
    // workgroups than a few per CU leave the chip idle -- P = 4 from 1 024 workgroups of it (8 rows: P = 2, the accumulators of
    // 4 pairs x 8 rows would not fit beside the codes)
    const int per1 = a.mode == AF_SWIGLU ? 4 : 8;
    constexpr int PW = TC == 0 ? 1 : (R == 8 ? 2 : 4);  // (mixed widths: the three bodies of a column take P = 1)
    const dim3 block(256);
    if (PW > 1 && cols >= (int64_t)1024 * per1 * PW) {
        const dim3 grid((unsigned)((cols + per1 * PW - 1) / (per1 * PW)));
        hipLaunchKernelGGL((affine_proj_kernel<TC, R, PW>), grid, block, 0, stream, a, k);
    } else {
        const dim3 grid((unsigned)((cols + per1 - 1) / per1));
        hipLaunchKernelGGL((affine_proj_kernel<TC, R, 1>), grid, block, 0, stream, a, k);
    }
}

template <int TC>
void launch_rows(const AffineProjArgs& a, int k, int64_t cols, hipStream_t stream)
{
    if (a.rows == 1) launch_instance<TC, 1>(a, k, cols, stream);
    else if (a.rows <= 4) launch_instance<TC, 4>(a, k, cols, stream);
    else launch_instance<TC, 8>(a, k, cols, stream);
}

}  // namespace

bool ggml_affine_type(uint32_t type)
{
    return type == GGML_Q4_0 || type == GGML_Q4_1 || type == GGML_Q5_0 || type == GGML_Q5_1 || type == GGML_Q5_K;
}

int affine_code_bits(uint32_t type) { return code_bits(type); }

QPlanes repack_affine32(uint32_t type, const uint8_t* blocks, int n, int k)
{
    if (!ggml_affine_type(type)) throw std::runtime_error(std::string("not an affine-32 matrix type: ") + ggml_type_name(type));
    int64_t be = 0, bb = 0;
    ggml_block_geometry(type, &be, &bb);
    if (n < 0 || k < 0 || k % be) throw std::runtime_error(std::string(ggml_type_name(type)) + " matrix with k % " + std::to_string(be) + " != 0");
    QPlanes p;
    const int64_t runs = (int64_t)n * (k / 32);
    const bool five = code_bits(type) == 5;
    p.plane[0].resize((size_t)runs * 16);
    if (five) p.plane[1].resize((size_t)runs * 4);
    p.plane[2].resize((size_t)runs * 8);
    uint8_t* nib = p.plane[0].data();
    uint32_t* high = five ? reinterpret_cast<uint32_t*>(p.plane[1].data()) : nullptr;
    float* ab = reinterpret_cast<float*>(p.plane[2].data());
    auto f16 = [](const uint8_t* src) {
        uint16_t h;
        std::memcpy(&h, src, 2);
        return f16_to_f32(h);
    };
    if (type == GGML_Q5_K) {
        for (int64_t b = 0; b < runs / 8; ++b) {
            const uint8_t* src = blocks + b * 176;
            const float d = f16(src), dmin = f16(src + 2);
            const uint8_t *qh = src + 16, *qs = src + 48;
            for (int s = 0; s < 8; ++s) {  // sub-block s: nibble half s % 2 of qs chunk s / 2, bit s of every qh byte
                const int64_t run = b * 8 + s;
                uint8_t sc, m;
                q4k_scale_min(s, src + 4, &sc, &m);
                ab[2 * run] = d * (float)sc;
                ab[2 * run + 1] = -(dmin * (float)m);
                const uint8_t* chunk = qs + (s / 2) * 32;
                auto code = [&](int l) { return (uint8_t)((s & 1) ? (chunk[l] >> 4) : (chunk[l] & 0xF)); };
                uint32_t word = 0;
                for (int e = 0; e < 32; ++e) word |= (uint32_t)((qh[e] >> s) & 1) << e;
                for (int i = 0; i < 16; ++i) nib[run * 16 + i] = (uint8_t)(code(i) | (code(i + 16) << 4));
                high[run] = word;
            }
        }
        return p;
    }
    const bool has_m = type == GGML_Q4_1 || type == GGML_Q5_1;
    const int qh_at = has_m ? 4 : 2, qs_at = qh_at + (five ? 4 : 0);
    for (int64_t run = 0; run < runs; ++run) {
        const uint8_t* src = blocks + run * bb;
        const float d = f16(src);
        ab[2 * run] = d;
        ab[2 * run + 1] = has_m ? f16(src + 2) : (five ? -16.0f : -8.0f) * d;
        if (five) std::memcpy(&high[run], src + qh_at, 4);
        std::memcpy(nib + run * 16, src + qs_at, 16);
    }
    return p;
}

hipError_t launch_affine_proj(const AffineProjArgs& a, hipStream_t stream)
{
    if (a.rows < 1 || a.rows > 8 || a.mode < AF_PLAIN || a.mode > AF_SWIGLU || !a.X || (a.ldx & 3) || (reinterpret_cast<uintptr_t>(a.X) & 15))
        return hipErrorInvalidValue;
    const int mats = a.mode == AF_QKV ? 3 : (a.mode == AF_SWIGLU ? 2 : 1);
    int k = 0, tc = -1;
    int64_t cols = 0;
    for (int i = 0; i < mats; ++i) {
        const QMat& W = a.W[i];
        if (W.n < 0 || (W.n == 0 && a.mode != AF_QKV)) return hipErrorInvalidValue;
        if (W.n == 0) continue;
        const int bits = code_bits(W.type);
        if (bits == 0 || W.k < 32 || W.k % 32 || (k && W.k != k) || !W.q || !W.s || (bits == 5 && !W.q2)) return hipErrorInvalidValue;
        k = W.k;
        tc = tc < 0 ? bits : (tc == bits ? tc : 0);
        cols += W.n;
        if (a.mode != AF_SWIGLU && !a.Y[i]) return hipErrorInvalidValue;
    }
    if (cols == 0 || (a.mode == AF_SWIGLU && (a.W[0].n != a.W[1].n || !a.Y[0] || a.R || a.bias)) || (a.mode == AF_QKV && a.R)) return hipErrorInvalidValue;
    if (a.gamma && (reinterpret_cast<uintptr_t>(a.gamma) & 15)) return hipErrorInvalidValue;
    if (a.mode == AF_SWIGLU) cols = a.W[0].n;
    switch (tc) {
    case 4: launch_rows<4>(a, k, cols, stream); break;
    case 5: launch_rows<5>(a, k, cols, stream); break;
    case 8: launch_rows<8>(a, k, cols, stream); break;
    default: launch_rows<0>(a, k, cols, stream);
    }
    return hipGetLastError();
}

hipError_t launch_affine_dequant(const QMat& W, float* out, hipStream_t stream)
{
    if (!ggml_affine_type(W.type) || W.k % 32 || (reinterpret_cast<uintptr_t>(out) & 15)) return hipErrorInvalidValue;
    const int64_t halves = (int64_t)W.n * (W.k / 32) * 2;
    if (halves < 1) return hipSuccess;
    const unsigned grid = (unsigned)std::min<int64_t>((halves + 255) / 256, 16384);
    hipLaunchKernelGGL(affine_dequant_kernel, dim3(grid), dim3(256), 0, stream, W, out);
    return hipGetLastError();
}

hipError_t launch_affine_embed(const uint32_t* ids, int n, const QMat& table, float* out, hipStream_t stream)
{
    if (!ggml_affine_type(table.type) || table.k % 32) return hipErrorInvalidValue;
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(affine_embed_kernel, dim3((unsigned)n), dim3(256), 0, stream, ids, table, out);
    return hipGetLastError();
}

}  // namespace kjarni
