// Batched scoring (LlmModel::score_batch): the plan that packs many sequences into chunks and computes a token prefix shared by
// neighbouring sequences once, the attention kernel a remainder uses to see its prefix, and the gather + final norm that
// brings only the scored rows to the vocabulary head.  Kernels: score_batch_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "decoder_embed_kernels.h"

namespace kjarni {

// One 32-query block of a remainder: its rows are `first` .. `first + len - 1` of the chunk, the block's queries start at row
// `q0` of the remainder, and the `prefix_len` rows from `prefix_first` stand in front of it as keys.
struct PrefixBlock {
    int32_t first, q0, len, prefix_first, prefix_len;
};

// Sequences [first_seq, first_seq + n_seq) share their first `prefix` tokens, which are computed once.
struct ScoreGroup {
    int chunk = 0, first_seq = 0, n_seq = 0, prefix = 0;
};

struct ScoreChunk {
    int first_seq = 0, n_seq = 0, rows = 0;
    std::vector<EmbedBlock> vec, mfma;  // plain sequences and prefixes (embed_plan_host's rule)
    std::vector<PrefixBlock> prefix;    // remainders
    std::vector<int32_t> row_tok;       // [rows]: the index in `ids` of the token each row computes
    std::vector<int32_t> row_pos;       // [rows]: that token's position in its sequence
    // one entry per scored position, in sequence order then position order: the chunk row of position pos - 1, the target
    // ids[pos], and the slot in the flat outputs
    std::vector<int32_t> gather_src, gather_tgt, gather_slot;
};

struct ScorePlan {
    std::vector<ScoreChunk> chunks;
    std::vector<ScoreGroup> groups;
    int64_t rows = 0, saved = 0;  // rows the chunks compute; sum of (members - 1) * prefix over the groups
};

// The rule (pure host code).  Sequence b is ids[offsets[b], offsets[b + 1]) with scored positions [firsts[b], len_b).  Walking in
// order, a sequence gathers the neighbours behind it while the prefix q = min(prefix so far, firsts[j], common prefix with
// sequence j) stays at least min_shared, the group's rows q + sum(len - q) fit one chunk and every remainder len - q stays below
// 256 rows; two or more members form a group (prefix rows first, then each remainder), else the sequence stays plain.  Units
// go greedily, in order, into chunks of at most kEmbedChunkRows rows.  Throws InvalidConfig naming the argument and the sequence
// for offsets that decrease, a length outside 2 .. kEmbedChunkRows and firsts[b] outside [1, len_b).
ScorePlan score_plan_host(const uint32_t* ids, const int32_t* offsets, const int32_t* firsts, int B, int head_dim, int min_shared);

// The plan of LlmModel::answer_logits_batch: score_plan_host's rule (packing, grouping, block tables, rows and saved) with
// firsts[b] = len_b - 1, so that a shared prefix never contains a sequence's last token.  The gather table differs: one entry per
// sequence, in order -- gather_src the chunk row of the sequence's last token (always a row of its own: a plain sequence's or a
// remainder's last row), gather_slot the sequence's index; gather_tgt stays empty.  Throws as score_plan_host does.
ScorePlan answer_plan_host(const uint32_t* ids, const int32_t* offsets, int B, int head_dim, int min_shared);

// packed_attention_kernel (decoder_embed_kernels.hip) over a virtual sequence: the keys of a block are its prefix rows, then the
// remainder's own rows; the query at remainder row t sees virtual keys 0 .. prefix_len + t.  Tiles start at virtual key 0 in
// steps of 64, so a remainder's rows are what launch_packed_causal_attention's vector kernel gives on the concatenation, bit
// for bit.  No row outside the prefix and the remainder is loaded.  Same head_dim and alignment rules.
hipError_t launch_packed_prefix_attention(const float* q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                                          const PrefixBlock* blocks, int n_blocks, int heads, int head_dim, int kv_group, float* ctx,
                                          int64_t ldc, hipStream_t stream);

// out[j, :] = norm(x[src[j], :]) for j < n, out rows ldo floats apart.  beta null: RMSNorm with rmsnorm_kernel's summation order (as
// last_token_pool_kernel follows it); beta given: launch_layernorm's arithmetic.  One workgroup per output row; hidden <= 16384.
hipError_t launch_score_gather_norm(const float* x, int64_t ldx, const int32_t* src, int n, int hidden, const float* gamma, const float* beta,
                                    float eps, float* out, int64_t ldo, hipStream_t stream);

}  // namespace kjarni
