// Launchers of llm_kernels.hip (conventions of kernels.h: enqueue on `stream`, no allocation, no sync).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kjarni {

// Y = epi(norm?(X) W^T + b) for up to 8 rows; W (and W2) are f32 or bf16 [n_out, k] row-major, k % 8 == 0.
struct LlmGemvArgs {
    const float* X = nullptr;
    int64_t ldx = 0;
    int rows = 0;
    const float* gamma = nullptr;  // non-null: RMS-normalise the rows first (LayerNorm when `layernorm` is set)
    float eps = 0.0f;
    int layernorm = 0;             // GPT-2: (x - mean) / sqrt(var + eps) * gamma + beta instead of RMSNorm
    const float* beta = nullptr;
    int gelu_tanh = 0;             // epilogue gelu_tanh(x.W + b) (GPT-2's c_fc; only after LayerNorm, no segments)
    const void* W = nullptr;
    const void* W2 = nullptr;      // SwiGLU `up` matrix
    int bf16 = 0;
    int swiglu = 0;
    const float* bias = nullptr;
    const float* R = nullptr;      // non-null: + residual
    int64_t ldr = 0;
    int n_out = 0, k = 0;
    int seg_q = 0, seg_kv = 0;     // seg_q > 0: [0,seg_q) -> Y0, then two seg_kv-wide segments -> Y1, Y2 at row row_off + r
    float* Y0 = nullptr;
    int64_t ldy0 = 0;
    float *Y1 = nullptr, *Y2 = nullptr;
    int64_t ldy12 = 0;
    int row_off = 0;
    const int* row_off_ptr = nullptr;
    // att_splits > 0 (only where llm_gemv_merges_attention() says so): X is not the context row but the decode attention's
    // slabs [k / att_head_dim heads][att_splits][att_head_dim + 4] (whisper_kernels.hip), merged while the weights stream in
    int att_splits = 0, att_head_dim = 0;
    float* norm_out = nullptr;     // rows == 1 with gamma (only where llm_gemv_streams()): the normalised row is also stored here
};
hipError_t launch_llm_gemv(const LlmGemvArgs& args, hipStream_t stream);
// The kernel launch_llm_gemv takes for these arguments and the form it takes it in (the launcher's own decision: it calls this).
// stream: llm_gemv_stream_kernel (one row, K = 2048 / 4096 / 8192); splitk: llm_gemv_splitk_kernel (one row, K over the waves of a
// workgroup); one: llm_gemv1_kernel (one row staged in LDS, cache segments); generic: llm_gemv_kernel (a wave per column, 1-8 rows).
enum : int { LLM_GEMV_STREAM = 0, LLM_GEMV_SPLITK = 1, LLM_GEMV_ONE = 2, LLM_GEMV_GENERIC = 3 };
struct LlmGemvRoute {
    int kernel = LLM_GEMV_GENERIC;
    int ch = 0;              // stream: 512-column pieces of K (4 / 8 / 16); splitk: 8-column chunks per lane (1 / 2 / 4 / 8); else 0
    int wide = 0;            // stream: 16 loads per lane in flight; splitk: 16 waves per workgroup
    int threads = 256;       // per workgroup: 256, 512 (stream) or 1024 (splitk, wide)
    int loop = 0;            // stream: the grid does not cover the columns, every wave walks several batches
    int rows_per_batch = 1;  // weight rows (columns of Y) per wave and batch (stream, one, generic) or per workgroup (splitk)
    int workgroups = 0;
};
LlmGemvRoute llm_gemv_route(const LlmGemvArgs& args);
// One row, + residual, no norm: can the projection merge `splits` attention slabs of `head_dim`-wide heads itself?
bool llm_gemv_merges_attention(int k, int splits, int head_dim);
// Does a one-row projection with these sizes take the weight-streaming kernel (which honours norm_out)?
bool llm_gemv_streams(int k, const void* W, const void* W2);

// One new token: RMSNorm + Q|K|V projection + RoPE in one launch; Q -> Q[n_heads*head_dim], K / V -> row `pos`
// (or *pos_ptr) of the caches [*, n_kv_heads*head_dim].  W is the fused [Q;K;V] matrix.
// embed_ids != null (only where llm_qkv_rope_embeds() says so): the input row is gathered from the embedding `table` (row
// *embed_ids, the weights' dtype; an id >= vocab leaves zeros) instead of read from X, and stored to x_raw_out (the residual stream).
hipError_t launch_llm_qkv_rope(const float* X, const float* gamma, float eps, const void* W, int bf16, const float* bias, int k,
                               int n_heads, int n_kv_heads, int head_dim, const float* cos_t, const float* sin_t, float* Q, float* Kc,
                               float* Vc, int pos, const int* pos_ptr, hipStream_t stream, const uint32_t* embed_ids = nullptr,
                               const void* table = nullptr, int vocab = 0, float* x_raw_out = nullptr);
bool llm_qkv_rope_embeds(int k, const float* gamma, const void* W, const void* table);
// The kernel launch_llm_qkv_rope takes (its own decision): a workgroup per pair of columns with `ch` 8-column chunks per lane
// (1 / 2 / 4), or the weight-streaming form (a wave per pair, ch = k / 512), the latter with or without the embedding gather.
enum : int { LLM_QKV_PAIR = 0, LLM_QKV_STREAM = 1, LLM_QKV_STREAM_EMBED = 2 };
struct LlmQkvRopeRoute {
    int kernel = LLM_QKV_PAIR, ch = 0, workgroups = 0;
};
LlmQkvRopeRoute llm_qkv_rope_route(int k, const float* gamma, const void* W, int n_heads, int n_kv_heads, int head_dim,
                                   const uint32_t* embed_ids);

// Prefill: Y[M, N] = A[M, K] . W[N, K]^T + bias (+ R) on the fp32 matrix cores, W bf16 or f32; K % 32 == 0.  R may alias Y.
// split_scratch (prefill_gemm_scratch_floats() floats, or null): short prompts split K over up to 8 workgroups per tile.
hipError_t launch_prefill_gemm(const float* A, int64_t lda, const void* W, int bf16, const float* bias, const float* R, int64_t ldr, float* Y,
                               int64_t ldy, int M, int N, int K, hipStream_t stream, float* split_scratch = nullptr,
                               float* silu_gate = nullptr);  // silu_gate: [M, N] gate activations, overwritten with silu(gate) * (this product)
size_t prefill_gemm_scratch_floats(int max_rows, int max_n);
// The number of K slices launch_prefill_gemm takes for these arguments (1: the unsplit kernel, whatever the scratch): the
// launcher's own decision, for callers that report it.
int prefill_gemm_launch_ksplit(const float* bias, const float* R, int64_t ldr, const float* Y, int64_t ldy, int M, int N, int K,
                               const float* split_scratch);
// The epilogue of a split launch: Y = the ksplit partial slabs [ksplit][M][N] added in slice order (+ bias) (+ R), or with silu_gate
// the SwiGLU product into the gate buffer.  For the GEMMs that share the slab layout (launch_prefill_gemm, launch_prefill_gemm_fp8).
hipError_t launch_prefill_splitk_reduce(const float* partials, int ksplit, const float* bias, const float* R, int64_t ldr, float* Y, int64_t ldy,
                                        int M, int N, float* silu_gate, hipStream_t stream);
// bf16 -> f32 copy of n values (n % 8 == 0): long prompts run the f32 tile GEMM (gemm.hip) on a widened weight matrix.
hipError_t launch_widen_bf16(const void* src, float* dst, size_t n, hipStream_t stream);

// Prefill: causal grouped-query attention of `rows` new rows (positions base .. base + rows - 1) over the cache rows
// 0 .. base + rows - 1; head_dim in {16, 32, 64, 128}.
bool prefill_attention_supported(int head_dim);
// The kernel launch_prefill_attention takes for these arguments: 0 the vector kernel, 1 the matrix-core kernel (its own decision).
int prefill_attention_route(const float* q, int64_t ldq, int rows, const float* K, int64_t ldk, const float* V, int64_t ldv, int head_dim);
hipError_t launch_prefill_attention(const float* q, int64_t ldq, int rows, const float* K, int64_t ldk, const float* V, int64_t ldv, int base,
                                    int heads, int head_dim, int kv_group, float* ctx, int64_t ldc, hipStream_t stream);

// Prefill: gate = silu(gate) * up (n multiple of 4).
hipError_t launch_swiglu_mul(float* gate, const float* up, size_t n, hipStream_t stream);

// In-place RoPE on `rows` rows of [n_heads * head_dim]; cos/sin tables are [max_pos, head_dim/2].
// at_cache_row: row r of the call lives at row (pos + r) of x (the KV cache), else at row r.
hipError_t launch_rope(float* x, int64_t ldx, int rows, int n_heads, int head_dim, const float* cos_t, const float* sin_t, int pos,
                       const int* pos_ptr, int at_cache_row, hipStream_t stream);
hipError_t launch_rmsnorm(const float* x, const float* gamma, float eps, int rows, int hidden, float* out, hipStream_t stream);
// Qwen3: per-head RMSNorm + RoPE in place, Q heads and K heads in one launch.  Row r sits at position p = (*pos_ptr | pos) + r
// (pos_ptr is read on the device: graph replay); each head vector x [head_dim] becomes (x / sqrt(mean(x^2) + eps)) * gamma,
// then its pairs (i, i + head_dim/2) are rotated by row p of the tables.  Q row r is row r of q; K row r is row p of k when
// k_at_cache_row, else row r.  gamma_q / gamma_k are [head_dim]; head_dim even and <= 128 (one wave per head).
hipError_t launch_qk_norm_rope(float* q, int64_t ldq, float* k, int64_t ldk, int rows, int n_heads, int n_kv_heads, int head_dim,
                               const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t, int pos,
                               const int* pos_ptr, int k_at_cache_row, hipStream_t stream);
hipError_t launch_llm_embed(const uint32_t* ids, int n, int hidden, int vocab, const void* table, int bf16, float* out,
                            hipStream_t stream);
// GPT-2: out[s] = table[ids[s]] + pos_table[p + s] for n rows, p = *pos_ptr when pos_ptr is non-null (graph replay), else pos;
// both tables in the weights' dtype, pos_table [max_pos, hidden].
hipError_t launch_llm_embed_pos(const uint32_t* ids, int n, int hidden, int vocab, const void* table, const void* pos_table, int max_pos,
                                int bf16, int pos, const int* pos_ptr, float* out, hipStream_t stream,
                                const int* row_pos = nullptr);  // given (lanes): row s sits at position row_pos[s]
// In place x = gelu_tanh(x) (activations.rs:62-66) over n floats, n % 4 == 0: the prompt route's c_fc epilogue where the GEMM has none.
hipError_t launch_gelu_tanh(float* x, size_t n, hipStream_t stream);
// argmax (last maximum wins); best_scratch: one zero-initialised u64 (re-zeroed by the call); history/count/pos may be null.
// The tie rule (argmax_key: the last maximum wins, +0.0 == -0.0, NaN lowest) lives in ONE kernel, argmax_partial_kernel, a row
// per blockIdx.y: launch_argmax, launch_lane_pick and launch_lookup_pick are grids over it, each followed by its own finalize.
hipError_t launch_argmax(const float* logits, int vocab, unsigned long long* best_scratch, int32_t* out, int32_t* history, int* count,
                         int* pos, hipStream_t stream);

// ---- lanes: sequences decoded in lock step, 1..kMaxLanes on the GEMV kernels (LlmModel::generate_lanes) and 9..kMaxWideLanes on
// the prompt GEMM (LlmModel::generate_wide; 64 = one M-tile of it: every width up to it streams the weights once per step) ----------
constexpr int kMaxLanes = 8, kMaxWideLanes = 64, kMaxLaneStops = 16;
// Everything the next lock-step step needs, on the device (so the step replays as a captured graph); the host reads it back
// and rewrites it between bursts of steps.  One definition, two layouts: N = 8 and N = 64.
template <int N>
struct LlmLaneStateT {
    int32_t token[N];  // the lane's next input token
    int32_t pos[N];    // its position = the lane's cache length
    int32_t live[N];   // 0: frozen (finished, or no prompt) -- the step writes nothing for it
    int32_t count[N];  // tokens picked for the lane's current request (history entries)
    int32_t limit[N];  // picks after which the lane is done (max_new_tokens and the context limit)
    int32_t n_stop[N];
    int32_t stop[N][kMaxLaneStops];  // picking one of these ends the lane
};
using LlmLaneState = LlmLaneStateT<kMaxLanes>;
using LlmWideState = LlmLaneStateT<kMaxWideLanes>;
// Either layout by field, passed by value: what the lane launchers and the pick's finalize kernel take.  Made from a state in
// device memory (only addresses are formed) or from its host mirror.
struct LaneStateRef {
    int32_t *token = nullptr, *pos = nullptr, *live = nullptr, *count = nullptr, *limit = nullptr, *n_stop = nullptr;
    int32_t (*stop)[kMaxLaneStops] = nullptr;
    int width = 0;  // the layout's lanes: kMaxLanes or kMaxWideLanes
    LaneStateRef() = default;
    template <int N>
    LaneStateRef(LlmLaneStateT<N>* s)
        : token(s->token), pos(s->pos), live(s->live), count(s->count), limit(s->limit), n_stop(s->n_stop), stop(s->stop), width(N)
    {
    }
    // the layout of `width` lanes at `base` (null for any other width)
    static LaneStateRef at(void* base, int width)
    {
        if (width == kMaxLanes) return LaneStateRef(static_cast<LlmLaneState*>(base));
        if (width == kMaxWideLanes) return LaneStateRef(static_cast<LlmWideState*>(base));
        return LaneStateRef();
    }
};
// launch_llm_gemv for 2-8 independent rows: the multi-row weight-streaming kernel where llm_gemv_lanes_takes() (k >= 512,
// 16-byte aligned operands), else launch_llm_gemv's one-wave-per-column kernel; *streamed (may be null) says which ran.
bool llm_gemv_lanes_takes(const LlmGemvArgs& args);
// The form of llm_gemv_lanes_kernel launch_llm_gemv_lanes takes (its own decision; taken == 0: it falls back to launch_llm_gemv and
// the other fields stay 0): slices of ch * 512 columns of K, ns of them, cpw columns per wave and batch (wide: more than one).
struct LlmGemvLanesRoute {
    int taken = 0, ch = 0, ns = 0, wide = 0, cpw = 0, workgroups = 0;
};
LlmGemvLanesRoute llm_gemv_lanes_route(const LlmGemvArgs& args);
hipError_t launch_llm_gemv_lanes(const LlmGemvArgs& args, hipStream_t stream, int* streamed);
// qkv [lanes, (n_heads + 2 n_kv_heads) * head_dim]: Q rotated in place at state.pos[lane], K rotated (rotate == 0: copied) and V
// copied to row pos[lane] of cache + lane * lane_stride; frozen lanes and positions >= capacity write nothing.  A workgroup per
// lane; lanes > state.width is refused (as by every launcher that takes the view).
hipError_t launch_lane_rope_scatter(float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim, const float* cos_t,
                                    const float* sin_t, float* k_cache, float* v_cache, int64_t lane_stride, int capacity,
                                    LaneStateRef state, int rotate, hipStream_t stream);
// The same for Qwen3: Q and K are RMS-normalised per head (gamma_q / gamma_k [head_dim], eps) before the rotation.
hipError_t launch_lane_qk_norm_rope_scatter(float* qkv, int64_t ld, int lanes, int n_heads, int n_kv_heads, int head_dim,
                                            const float* gamma_q, const float* gamma_k, float eps, const float* cos_t, const float* sin_t,
                                            float* k_cache, float* v_cache, int64_t lane_stride, int capacity, LaneStateRef state,
                                            hipStream_t stream);
// Per-lane argmax over rows [first_lane, first_lane + lanes) of logits [state.width, ld] (argmax_partial_kernel: last maximum
// wins) for the live lanes, then the finalize: appended to history[lane, count], count (and pos when `advance`: after a step)
// + 1, live cleared on a stop id / the limit / a full cache, else token = the pick.  best_scratch: state.width zero-initialised
// u64 (re-zeroed by the call).
hipError_t launch_lane_pick(const float* logits, int64_t ld, int vocab, int lanes, int first_lane, unsigned long long* best_scratch,
                            LaneStateRef state, int32_t* history, int hist_stride, int capacity, int advance, hipStream_t stream);
// Shared prompt prefix: `count` floats from the start of every layer's single-sequence K and V cache into a lane's caches, one
// launch for all layers.  table[layer] (device memory) = the source pointers and the lane-0 destination pointers; dst_offset =
// the lane's offset in floats.  Bit-exact; 16-byte vector copies where source and destination are 16-byte aligned, 4-byte
// copies otherwise (and for the tail of a count that is no multiple of 4).
struct LlmKvCopyPair {
    const float* src_k;
    float* dst_k;
    const float* src_v;
    float* dst_v;
};
hipError_t launch_kv_prefix_copy(const LlmKvCopyPair* table, int layers, int64_t dst_offset, int64_t count, hipStream_t stream);

// ---- prompt-lookup decoding (LlmModel::generate_lookup): draft from the sequence's own history, verify in one multi-row step
constexpr int kLookupMaxDraft = 7, kLookupMaxNgram = 4;
struct LlmLookupState {
    int32_t n;          // history length: the prompt, then every pick; the last entry is the token that is not in the cache yet
    int32_t steps;      // verify steps since the host last zeroed it = entries of the step log
    int32_t m;          // draft length of the step in flight (rows 1..m of its ids)
    int32_t a;          // drafted tokens the last step accepted
    int32_t picks[8];   // its picks p_0..p_a
};
// The draft rule (longest match of ngram_min..ngram_max tokens against the history's suffix, then the longest continuation
// up to draft_tokens <= rows - 1, then the latest) on history[0, state->n): ids[0] = the last token, ids[1..m] = the draft, the
// other rows repeat the last of them; state->m = m.  One launch of one workgroup, order-free reduction.
hipError_t launch_lookup_draft(const int32_t* history, LlmLookupState* state, int ngram_max, int ngram_min, int draft_tokens, int rows,
                               uint32_t* ids, hipStream_t stream);
// The verify pick on logits [rows, ld] (two launches): per-row argmax p_i (last maximum wins), a = the longest prefix with
// ids[1 + i] == p_i, i < a <= state->m; p_0..p_a go to state->picks and history[state->n ..] (may be null), state->n and *pos
// advance by a + 1, (m, a) goes to log[2 * state->steps ..] (may be null).  best_scratch: 8 zero-initialised u64 (re-zeroed).
hipError_t launch_lookup_pick(const float* logits, int64_t ld, int vocab, int rows, const uint32_t* ids, unsigned long long* best_scratch,
                              LlmLookupState* state, int32_t* history, int hist_cap, int* pos, int32_t* log, int log_cap, hipStream_t stream);

// ---- scoring (LlmModel::score): per row of final-normed hidden states X[m, k] the log-sum-exp of its `vocab` logits X . W^T,
// the arg-max (last maximum wins, launch_argmax's rule) and the logit of targets[row]; outputs logprob = target - lse,
// top, top_logprob = best - lse and lse, each [m] and each may be null (targets null: no logprob).
// The fused route: the head on the fp32 matrix cores without storing the logits (llm_score_head_kernel + llm_score_merge_kernel),
// W [vocab, k] f32 or bf16 row-major.  Needs k % 32 == 0, ldx % 4 == 0 and 16-byte aligned X and W (llm_score_head_takes).
// slab_tiles: 64-wide vocabulary tiles per workgroup, 0 = chosen so that the grid covers the chip; scratch:
// score_head_scratch_bytes(m, vocab, slab_tiles) bytes, no initialisation needed.
bool llm_score_head_takes(const float* X, int64_t ldx, const void* W, int bf16, int k);
int score_head_slab_tiles(int m, int vocab, int slab_tiles);  // the slab width the launch uses
size_t score_head_scratch_bytes(int m, int vocab, int slab_tiles);
hipError_t launch_score_head(const float* X, int64_t ldx, int m, const void* W, int bf16, int vocab, int k, const uint32_t* targets,
                             int slab_tiles, void* scratch, float* logprob, uint32_t* top, float* top_logprob, float* lse, hipStream_t stream);
#ifndef KJARNI_SCORE_TOPK_MAX
#define KJARNI_SCORE_TOPK_MAX 8  // (include/kjarni_hip.h)
#endif
// Top-k (LlmModel::score_topk): besides logprob and lse, the top_k (1 .. KJARNI_SCORE_TOPK_MAX, <= vocab) largest logits of every
// row as topk_ids / topk_logprob [m, top_k] row-major, in descending argmax_key order (value, then the larger index; slot 0 is
// launch_score_head's top / top_logprob).  Every lane of the head kernel keeps a sorted list of keys next to its running sums;
// logprob, lse and slot 0 are bit-identical to launch_score_head's with the same slab_tiles.  scratch:
// score_head_topk_scratch_bytes bytes.
size_t score_head_topk_scratch_bytes(int m, int vocab, int slab_tiles, int top_k);
hipError_t launch_score_head_topk(const float* X, int64_t ldx, int m, const void* W, int bf16, int vocab, int k, const uint32_t* targets,
                                  int slab_tiles, int top_k, void* scratch, float* logprob, uint32_t* topk_ids, float* topk_logprob, float* lse,
                                  hipStream_t stream);
// The rows route: the same outputs from up to 8 materialised logits rows [rows, ld] (llm_score_rows_kernel).
hipError_t launch_score_rows(const float* logits, int64_t ld, int rows, int vocab, const uint32_t* targets, float* logprob, uint32_t* top,
                             float* top_logprob, float* lse, hipStream_t stream);
hipError_t launch_score_rows_topk(const float* logits, int64_t ld, int rows, int vocab, const uint32_t* targets, int top_k, float* logprob,
                                  uint32_t* topk_ids, float* topk_logprob, float* lse, hipStream_t stream);

// ---- sampled decoding: the O(vocab) part on the device (llm_kernels.hip) ----------------------------------------------
struct SampleHeader {   // 32 bytes, device memory mirrored to the host per sampled token
    float mx;           // maximum logit
    float sum;          // sum of exp(logit - mx) over the vocabulary (deterministic, not in index order)
    float floor;        // every token with logit >= floor is in the candidate list
    uint32_t count;     // tokens with logit >= floor (more than the capacity, or no cut -- then all of them: overflow is set)
    uint32_t overflow;  // 1: the list is not usable (too long, or no cut could be placed) -- fetch the logits
    uint32_t pad[3];
};
struct SampleCandidate {
    uint32_t token;
    float logit;
};
// One kernel family (sample_max / sample_hist / sample_compact, the row in blockIdx.y) makes the cut; the two launchers below
// are grids over it: this one a single row with a contiguous candidate list, launch_sample_candidates_rows up to 8 rows.
size_t sample_scratch_bytes();   // zero-initialised device scratch of launch_sample_candidates
// top_k < 0 / top_p < 0 / min_p < 0: that filter is off (as SamplingParams).
hipError_t launch_sample_candidates(const float* logits, int vocab, int64_t top_k, float top_p, float min_p, void* scratch,
                                    SampleHeader* header, SampleCandidate* candidates, int capacity, hipStream_t stream);
// Logits processors on the device.  State: counts[vocab] (occurrences of each token in the history), distinct[] (the tokens
// with a non-zero count) and *n_distinct, all zero-initialised and advanced by launch_token_counts for every token that
// joins the history; tokens[len] is the history itself, in order.  The repetition penalty is row 0 of
// launch_repetition_penalty_rows's kernel (a row 0 has no draft, so no ids).
hipError_t launch_token_counts(const int32_t* tokens, int n, int vocab, int* counts, int32_t* distinct, int* n_distinct, hipStream_t stream);
hipError_t launch_logits_processors(float* logits, int vocab, const int32_t* tokens, int len, const int* counts, const int32_t* distinct,
                                    const int* n_distinct, float repetition_penalty, int no_repeat_ngram, hipStream_t stream);

// ---- sampled prompt-lookup decoding (LlmModel::generate_lookup_sampled) ---------------------------------------------------------
// launch_sample_candidates's kernels over `rows` (1..8) logits rows of stride ld >= vocab: the same three launches with `rows`
// as the grid's y.  Row r uses scratch + r * sample_scratch_bytes() (sample_scratch_rows_bytes(rows) in all, zero-initialised),
// headers[r] and its own `capacity` candidate slots: per row the one-row launcher's contract, and -- the same code walking the
// row with the same 64 workgroups -- mx and sum bit-identical to it; an overflowing row reports its own count and touches no
// slot past its capacity and nothing of its neighbours.
// The slots are laid out in chunks of kSampleRowsChunk so that the first 512 candidates of all rows are contiguous: slot s of
// row r is entry sample_rows_slot(r, s) of `candidates` (sample_rows_entries(capacity) entries whatever `rows` is).  With the
// headers placed right in front, [8 headers | rows x 512 candidates] is ONE contiguous device-to-host copy; a row with more
// candidates has them in the later chunks.
constexpr int kSampleRowsChunk = 512, kSampleRowsMax = 8;
__host__ __device__ inline size_t sample_rows_slot(int row, int slot)
{
    return ((size_t)(slot / kSampleRowsChunk) * kSampleRowsMax + (size_t)row) * kSampleRowsChunk + (size_t)(slot % kSampleRowsChunk);
}
inline size_t sample_rows_entries(int capacity)
{
    return (size_t)((capacity + kSampleRowsChunk - 1) / kSampleRowsChunk) * kSampleRowsMax * kSampleRowsChunk;
}
size_t sample_scratch_rows_bytes(int rows);
hipError_t launch_sample_candidates_rows(const float* logits, int64_t ld, int rows, int vocab, int64_t top_k, float top_p, float min_p,
                                         void* scratch, SampleHeader* headers, SampleCandidate* candidates, int capacity, hipStream_t stream);
// The repetition penalty over the rows of a verify block: row r (it predicts the token after ids[0..r]) is penalised for the
// history that counts / distinct / n_distinct describe (up to and including ids[0]: launch_token_counts's state) plus
// ids[1..r], once per occurrence, bit-exact against apply_repetition_penalty on the concatenation.  One kernel serves this
// launcher (grid 16 x rows) and launch_logits_processors (one row); a `distinct` entry outside [0, vocab) is skipped.
hipError_t launch_repetition_penalty_rows(float* logits, int64_t ld, int rows, int vocab, const uint32_t* ids, const int* counts,
                                          const int32_t* distinct, const int* n_distinct, float penalty, hipStream_t stream);
// The host's decision of a sampled verify step: upload[0] = k (0..8) picks, upload[1..k] join history[state->n ..]; state->n and
// *pos advance by k.
hipError_t launch_lookup_commit(const int32_t* upload, LlmLookupState* state, int32_t* history, int hist_cap, int* pos, hipStream_t stream);

}  // namespace kjarni
