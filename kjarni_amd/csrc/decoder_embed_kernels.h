// Kernels of the decoder embedders (decoder_embed_kernels.hip): many sequences packed into one row block, causal attention
// that stops at the sequence boundaries, RoPE by a per-row position, and the last-token pool.  Host side: LlmModel::embed_batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace kjarni {

constexpr int kEmbedChunkRows = 2048;  // rows of the prompt workspace: the most a chunk packs, and the longest sequence

// One query block of packed_causal_attention: `first` = the sequence's first row in the chunk, `q0` = the block's first query
// row inside the sequence, `len` = the sequence's length.
struct EmbedBlock {
    int32_t first, q0, len;
};

// The packing rule (pure host code).  Sequences are packed greedily, in order, into chunks of at most kEmbedChunkRows rows and
// never straddle a chunk.  Per chunk the two block tables: a sequence of at least 256 rows with head_dim 64 or 128 puts one
// entry per 128 query rows into `mfma`, every other sequence one entry per 32 query rows into `vec`.
struct EmbedChunk {
    int first_seq = 0, n_seq = 0, rows = 0;  // sequences [first_seq, first_seq + n_seq), their rows in total
    std::vector<EmbedBlock> vec, mfma;
};
// Throws InvalidConfig naming lengths[i] for a length outside 1 .. kEmbedChunkRows.
std::vector<EmbedChunk> embed_plan_host(const int32_t* lengths, int n, int head_dim);
// Whether a sequence of `len` rows takes the matrix-core route (launch_prefill_attention's rule).
inline bool embed_seq_takes_mfma(int len, int head_dim) { return len >= 256 && (head_dim == 64 || head_dim == 128); }

// Causal grouped-query attention over packed rows.  q [T, ldq] (heads * head_dim used), K / V [T, ldk / ldv] (kv heads *
// head_dim used), ctx [T, ldc]; query row r of a sequence that starts at row f sees keys f .. r and nothing else.  `vec` /
// `mfma` are device tables of n_vec / n_mfma blocks (grid.x walks them; a route with no block is not launched).  No row of
// another sequence, and none at or past T, is loaded.  head_dim in {16, 32, 64, 128}; pointers 16-byte aligned, leading
// dimensions multiples of 4.  Arithmetic: prefill_attention_kernel / prefill_attention_mfma_kernel at base = 0.
hipError_t launch_packed_causal_attention(const float* q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                                          const EmbedBlock* vec, int n_vec, const EmbedBlock* mfma, int n_mfma, int heads, int head_dim,
                                          int kv_group, float* ctx, int64_t ldc, hipStream_t stream);

// launch_rope with row r rotated by row_pos[r] instead of pos + r (rows of x in place).
hipError_t launch_rope_rows(float* x, int64_t ldx, int rows, int n_heads, int head_dim, const float* cos_t, const float* sin_t,
                            const int32_t* row_pos, hipStream_t stream);
// launch_qk_norm_rope with row r at position row_pos[r]; its K heads are row r of k.
hipError_t launch_qk_norm_rope_rows(float* q, int64_t ldq, float* k, int64_t ldk, int rows, int n_heads, int n_kv_heads, int head_dim,
                                    const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                    const int32_t* row_pos, hipStream_t stream);

// out[b, :] = l2?(rmsnorm(x[seq_start[b + 1] - 1, :])) for b in [0, n_seq): rmsnorm_kernel's arithmetic, then x / ||x|| when
// ||x|| > 0.  One workgroup per sequence; hidden <= 16384.
hipError_t launch_last_token_pool(const float* x, int64_t ldx, const int32_t* seq_start, int n_seq, int hidden, const float* gamma, float eps,
                                  int normalize, float* out, hipStream_t stream);

}  // namespace kjarni
