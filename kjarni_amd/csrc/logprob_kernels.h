// Generation log-probabilities on the device (gfx950): what a decode step's logits row says about the token the step emitted.
//
//   partial   rows of logits [rows, ld] (a row per blockIdx.y, as the token-selection family), each row's vocabulary cut into
//             `slabs` slabs over blockIdx.x: per slab the maximum, the sum of exp(x - max) and the TOPK largest argmax keys go to
//             scratch; with raw_copy the same pass stores the row unchanged into a second buffer.
//   finish    one wave per row merges the row's slabs in a fixed order (the same call gives the same bits twice), reads the
//             chosen token and the record index from device memory and writes the record:
//             logprob = raw_logit[token] - lse, topk_ids[j], topk_logprob[j] = value_j - lse.
//
// The distribution is the log-softmax of the logits as the vocabulary head wrote them: a loop whose mask or processors edit the
// row in place runs the partial kernel (with raw_copy) before them and the finish kernel, on the copy, once the token is known.
// The top-k order is score_topk's (argmax_key: descending value, among equal logits the larger id first, +0.0 == -0.0, NaN
// lowest), so slot 0 is what launch_argmax picks on the same row.  No float atomics: every reduction runs lane -> wave ->
// workgroup -> slabs in one order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace kjarni {

constexpr int kLogprobMaxRows = 64;      // kMaxWideLanes: one row per lane of the widest step
constexpr int kLogprobMaxSlabs = 64;     // the finish kernel gives every slab of a row one lane of its wave
constexpr int kLogprobMinSlab = 1024;    // elements: one 16-byte load per thread of a 256-thread workgroup
constexpr int kLogprobGridTarget = 512;  // workgroups the slab rule aims at (two per CU of the 256)
constexpr int kLogprobTopkMax = 8;       // KJARNI_SCORE_TOPK_MAX

// The slab rule, in one place: slabs = min(kLogprobMaxSlabs, ceil(vocab / kLogprobMinSlab), max(1, ceil(kLogprobGridTarget /
// rows))), each slab a multiple of 4 elements long (the 16-byte loads), recounted over that length.  One row covers 64
// workgroups, 64 rows cover 512.
int token_logprob_slabs(int rows, int vocab);
int token_logprob_slab_len(int rows, int vocab);  // elements per slab (the last one may be shorter)
// Scratch of one launch pair over up to `rows` rows (no initialisation needed).
size_t token_logprob_scratch_bytes(int rows, int vocab);

struct TokenLogprobArgs {
    const float* logits = nullptr;  // [rows, ld], ld >= vocab
    int64_t ld = 0;
    int rows = 0, vocab = 0;
    int top_k = 0;                  // 0 .. kLogprobTopkMax, <= vocab; 0: the chosen token's logprob only
    const int32_t* live = nullptr;  // null, or [rows]: a row whose flag is 0 is neither read nor written
    void* scratch = nullptr;        // token_logprob_scratch_bytes(rows, vocab)
    float* raw_copy = nullptr;      // null, or [rows, ld_copy]: the partial pass stores the row's `vocab` logits here
    int64_t ld_copy = 0;
};

// The record of row r goes to index i = r * rec_stride + (count ? count[r * count_stride] : 0) + index_bias of logprob / lse and
// to [i, slots] of topk_ids / topk_logprob (slots >= top_k: the row pitch of the two); an index outside [r * rec_stride,
// r * rec_stride + rec_cap) writes nothing, nor does a row whose live flag is 0 or whose token is outside [0, vocab).
struct TokenLogprobRecord {
    const float* raw = nullptr;  // [rows, ld_raw]: where the chosen token's logit is read (the logits, or the partial's raw_copy)
    int64_t ld_raw = 0;
    // device: row r's chosen token at tokens[r * token_stride]; null: the row's own arg-max (slot 0), which is what launch_argmax
    // and the lane picks choose on the same row -- for a finish step that runs ahead of the pick on rows nothing has edited
    const int32_t* tokens = nullptr;
    int token_stride = 1;
    const int* count = nullptr;  // device, may be null
    int count_stride = 1, index_bias = 0;
    int rec_stride = 1, rec_cap = 1, slots = 0;
    float* logprob = nullptr;       // may be null, as every output
    uint32_t* topk_ids = nullptr;
    float* topk_logprob = nullptr;
    float* lse = nullptr;
};

hipError_t launch_token_logprob_partial(const TokenLogprobArgs& args, hipStream_t stream);
hipError_t launch_token_logprob_finish(const TokenLogprobArgs& args, const TokenLogprobRecord& rec, hipStream_t stream);

}  // namespace kjarni
