// LlmModel: a decoder-only transformer (Llama / Qwen2 / Qwen3 / Mistral layouts, and GPT-2) resident in HBM with an f32 KV cache,
// and the generation loop.  Qwen3 (safetensors only; a GGUF of that architecture is refused): Q and K are RMS-normalised per
// head before RoPE (launch_qk_norm_rope, one launch more per layer than the Llama step), there are no Q/K/V biases, and
// head_dim comes from the config, so the query / context width q_dim() = heads * head_dim may differ from hidden.
//
//   config + tensor names   crates/kjarni-models/src/models/llama/config.rs:98-330, qwen/config.rs:80-275
//   layer                   crates/kjarni-transformers/src/cpu/decoder/rope_decoder_layer.rs:18-41
//   model forward           crates/kjarni-models/src/models/llama/cpu_decoder.rs:142-219
//   generation loop         crates/kjarni-transformers/src/decoder/generator.rs:228-381 (DecodingStrategy::Greedy)
//   GPT-2                   crates/kjarni-models/src/models/gpt2/{config.rs:8-125, cpu_decoder.rs:180-394}
#pragma once
#include "device_arena.h"
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "encoder.h"
#include "fp8_kernels.h"
#include "generation_run.h"
#include "llm_kernels.h"
#include "quant_kernels.h"
#include "sampling.h"

namespace kjarni {

class SafeTensors;

struct LlmConfig {
    std::string model_type;
    int hidden = 0, layers = 0, heads = 0, kv_heads = 0, head_dim = 0, inter = 0, vocab = 0, max_pos = 0;
    float eps = 1e-5f, rope_theta = 500000.0f;
    bool tie_embeddings = true;
    bool has_rope_scaling = false;
    std::string rope_type;
    float rope_factor = 1.0f, rope_low = 1.0f, rope_high = 4.0f;
    int rope_original_max = 8192;
    std::vector<uint32_t> eos_ids;
    bool has_bos = false;
    uint32_t bos_id = 0;
    bool gpt2() const { return model_type == "gpt2"; }  // LayerNorm + biases, GELU MLP, learned positions, head tied to wte
    bool moe() const { return model_type == "qwen3_moe"; }  // Qwen3 in everything but the FFN: a router and E experts in the sparse layers
    bool qwen3() const { return model_type == "qwen3" || moe(); }  // per-head RMSNorm of Q and K before RoPE; head_dim set apart from hidden / heads
    // qwen3_moe: E experts of width moe_inter, k of them per token; layer i is sparse iff it is not in mlp_only_layers and
    // (i + 1) % sparse_step == 0, else a dense Qwen3 layer of `inter`
    int num_experts = 0, experts_per_tok = 0, moe_inter = 0, sparse_step = 1;
    bool norm_topk = false;
    std::vector<int> mlp_only_layers;
    bool sparse_layer(int i) const;
    int q_dim() const { return heads * head_dim; }  // the width of Q and of the attention's context rows (== hidden except for Qwen3)
    static LlmConfig from_json(const std::string& text);
};

// One request of LlmModel::generate_lanes: a prompt and the options generate() would take for it.
struct LaneRequest {
    std::vector<uint32_t> prompt;
    GenerateOptions options;
};

struct ConstraintView;  // constraint_kernels.h
struct ConstraintRow;
struct GrammarView;  // grammar_kernels.h
struct GrammarRow;
struct LaneAutomatonTable;  // lane_constraint_kernels.h
struct LlmLookupState;
struct SampleHeader;
struct LlmKvCopyPair;
struct EmbedBlock;   // decoder_embed_kernels.h
struct PrefixBlock;  // score_batch_kernels.h

#ifndef KJARNI_SCORE_TOPK_MAX
#define KJARNI_SCORE_TOPK_MAX 8  // (include/kjarni_hip.h): the most alternatives score_topk() returns per position
#endif
#ifndef KJARNI_HIP_SCORE_MIN_SHARED
#define KJARNI_HIP_SCORE_MIN_SHARED 2  // (include/kjarni_hip.h): LlmModel::kScoreMinShared, where the measured reason stands
#endif

// Prompt-lookup decoding: how the draft of a verify step is found in the sequence's own history.
struct LookupConfig {
    int draft_tokens = 7;  // 1..7 tokens drafted per step (a step verifies draft_tokens + 1 rows)
    int ngram_max = 3;     // 1..4: the longest suffix of the history that is matched
    int ngram_min = 1;     // 1..ngram_max: the shortest match that drafts anything
};
struct LookupStats {  // over the steps the host consumed
    uint64_t verify_steps = 0, drafted_tokens = 0, accepted_tokens = 0, single_row_steps = 0;
    void count(int rows, int drafted, int accepted)  // one consumed step of `rows` rows
    {
        ++(rows == 1 ? single_row_steps : verify_steps);
        drafted_tokens += (uint64_t)drafted;
        accepted_tokens += (uint64_t)accepted;
    }
};
// The draft rule on a host-side history (what the device kernel computes): the tokens drafted after `tokens`.
std::vector<uint32_t> lookup_draft_host(const uint32_t* tokens, size_t n, const LookupConfig& config);
void check_lookup_config(const LookupConfig& config);  // InvalidConfig naming the field
// Prefix reuse: how many cache rows a call may keep.  min(longest common prefix of the resident tokens and the prompt, limit);
// a caller that needs the logits of the last prompt token passes limit = n_prompt - 1, score() passes first - 1.
size_t prefix_keep_host(const uint32_t* resident, size_t n_resident, const uint32_t* prompt, size_t n_prompt, size_t limit);

class LlmModel {
public:
    // dir: a safetensors model directory, a `.gguf` file or a directory that holds one (gguf.h: resolve_gguf).
    // weights: 0 = as stored (BF16 stays bf16, everything else f32; GGUF Q8_0 / Q4_K / Q6_K matrices stay quantized), 1 = f32,
    // 2 = bf16 (f32 rounded to nearest even).
    static std::unique_ptr<LlmModel> load(const std::string& dir, int device, int weights, int max_context);
    ~LlmModel();
    LlmModel(const LlmModel&) = delete;
    LlmModel& operator=(const LlmModel&) = delete;

    const LlmConfig& config() const { return cfg_; }
    bool bf16() const { return bf16_; }
    size_t weight_bytes() const { return weight_bytes_; }
    // device bytes of the weights held in each GGML type (0 = F32, 30 = BF16, 8 / 12 / 14 = Q8_0 / Q4_K / Q6_K)
    uint64_t weight_bytes_of_type(int type) const { return type >= 0 && type < 32 ? bytes_by_type_[type] : 0; }
    bool quantized() const { return quant_; }
    const std::string& config_json() const { return config_json_; }  // config.json, or the config synthesized from GGUF metadata
    int context() const { return cache_cap_; }
    int cache_len() const { return cache_len_; }
    int device() const { return device_; }
    // A number no other model of this process has had (assigned at load, never reused): what a captured chain that holds another
    // model's pointers is keyed by -- an address can come back after a free, a serial cannot.
    uint64_t serial() const { return serial_; }
    // Prompt projections that ran the encoder's 128 x 128-tile GEMM since load (the other route is the 64 x 64 prompt kernel):
    // lets a test assert which route a geometry took.
    uint64_t tile_gemm_calls() const { return tile_gemm_calls_; }
    // A qwen3_moe directory checked on the host alone (config, every expert tensor's presence and shape, the refusals), before
    // load() touches a device; any other directory returns at once.  Throws what load() would.
    static void check_moe_checkpoint(const std::string& dir);
    // What sparse layer `layer` chose in its last pass: rows of k expert ids and weights.  Returns the rows recorded (the
    // caller's arrays hold moe_record_rows(layer) * k values); InvalidConfig for a dense layer or a dense model.
    int moe_record_rows(int layer) const;
    void moe_routing(int layer, int32_t* ids_out, float* weights_out);
    // Sampled decoding / logits processors: the O(vocab) work runs on the device and the host decides on a candidate list
    // (default); off = the logits travel to the host every token (the checker in tests).  The counters say how many tokens
    // were decided from candidates and how many needed the logits after all.
    void set_device_sampling(bool on) { device_sampling_ = on; }
    uint64_t tokens_from_candidates() const { return tokens_from_candidates_; }
    uint64_t tokens_from_logits() const { return tokens_from_logits_; }

    void reset();  // empty KV cache
    // ---- prefix reuse: the entry points keep the cache rows of the longest common prefix with what the cache holds -----------
    // Off (the default): generate(), generate_lookup(), generate_lookup_sampled() and score() empty the cache and prefill the
    // whole prompt.  On: they keep the rows of prefix_keep_host(resident tokens, prompt, limit) and forward only the rest, and
    // generate_lanes() prefills the prefix all its prompts share once, into the single-sequence cache, and copies its rows into
    // every lane that takes a request (launch_kv_prefix_copy).  Kept rows were computed by whichever route wrote them, so the
    // results are the no-reuse results inside the float bar.  The resident tokens are tracked whether the switch is on or off.
    void set_prefix_reuse(bool on) { prefix_reuse_ = on; }
    bool prefix_reuse() const { return prefix_reuse_; }
    // ---- FP8 checkpoints on the matrix cores (off by default; a no-op on a checkpoint that is not FP8) --------------------------
    // On: a prompt projection on the 64 x 64 route multiplies the FP8 codes themselves (launch_prefill_gemm_fp8) instead of
    // dequantizing the matrix into the f32 scratch first, and the wide bank takes the checkpoint: the wide step then writes Q, K
    // and V from their three matrices into the staging rows' column segments and rows_finish() runs on the same GEMM.  Off:
    // everything enqueued is what it was before the switch existed.  Flipping it drops the wide bank's captured graphs and ends
    // its session (lanes_begin(Bank::Wide) again).
    void set_fp8_matrix_cores(bool on);
    bool fp8_matrix_cores() const { return fp8_mc_; }
    // Prompt tokens whose rows were kept / computed by the calls that ran with reuse on, since load.
    uint64_t prefix_reused_tokens() const { return prefix_reused_; }
    uint64_t prefix_computed_tokens() const { return prefix_computed_; }
    // resident()[i] is the token whose K / V sit in row i of the single-sequence cache; size() <= cache_len() (rows past it
    // belong to tokens a loop computed and then discarded, or to test hooks that do not say what they fed).
    const std::vector<uint32_t>& resident() const { return resident_; }
    // Appends n tokens (fewer than 24: 8-row passes; more: the matrix-core route in 2 048-row chunks); the logits of the last
    // position stay on the device.
    void forward(const uint32_t* ids, int n);
    // Scoring: resets the cache, runs ids[0, n) through forward()'s routes and returns, for every position p in [first, n)
    // (1 <= first < n; entry p - first), log p(ids[p] | ids[0, p)), the arg-max token of that distribution and the arg-max's
    // log-probability (log_softmax_1d, sampling.rs:200-205); any output may be null.  Only the rows first - 1 .. n - 2 reach
    // the vocabulary head, score_head(): on the fp32 matrix cores without storing their logits (launch_score_head; f32 / bf16
    // heads with hidden % 32 == 0), else through the 8-row logits buffer of the verify step (launch_score_rows; quantized heads,
    // other geometries, or set_score_fused(false)).  The results stay on the device until one copy at the end.  Leaves the model as
    // reset(); forward(ids, n) does.  Throws InvalidConfig naming the argument, before any GPU work, for n < 2, first outside
    // [1, n), n > context() and an id >= vocab.
    void score(const uint32_t* ids, int n, int first, float* logprob_out, uint32_t* top_out, float* top_logprob_out);
    // score() with the top_k (1 .. KJARNI_SCORE_TOPK_MAX, <= vocab) most likely tokens of every scored position instead of the
    // arg-max alone: topk_ids_out / topk_logprob_out are [n - first, top_k] row-major, slot j the j-th largest logit (equal values:
    // the larger id first), slot 0 what score() returns as top / top_logprob.  Same sink, routes, chunks, prefix reuse, counters
    // and final state as score(); logprob_out is bit-identical to score()'s.  Any output may be null.
    void score_topk(const uint32_t* ids, int n, int first, int top_k, float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out);
    void set_score_fused(bool on) { score_fused_ = on; }
    // Head launches of score() by route since load.
    uint64_t score_fused_calls() const { return score_fused_calls_; }
    uint64_t score_rows_calls() const { return score_rows_calls_; }
    // ---- embedding: last-token pooling over a packed batch ---------------------------------------------------------------------
    // Sequence b is ids[offsets[b], offsets[b + 1]); out[b, :] = the final-normed hidden state of its last token, L2-normalised
    // when `normalize` (x / ||x|| when ||x|| > 0).  The sequences are packed, in order, into chunks of at most 2 048 rows
    // (embed_plan_host, decoder_embed_kernels.h) and every chunk runs prefill_rows()'s layer body (rows_qkv / rows_finish) once
    // over all its rows: the projections on the prompt GEMM routes, RoPE by each row's position in its own sequence, causal attention that stops at the
    // sequence boundaries; K and V live in two scratch buffers, not in the KV cache.  cache_len(), resident(), lanes, lookup
    // state, the logits and last_hidden() are left as they were.  Throws InvalidConfig naming the argument and the sequence, before
    // any GPU work, for non-monotone offsets, an empty sequence, an id >= vocab and a sequence longer than
    // embed_max_tokens(); GPT-2, quantized checkpoints and geometries forward() keeps off the matrix-core route are refused.
    // B == 0 writes nothing.
    void embed_batch(const uint32_t* ids, const int32_t* offsets, int B, bool normalize, float* out);
    int embed_max_tokens() const { return cache_cap_ < 2048 ? cache_cap_ : 2048; }
    // ---- scoring many sequences in one packed pass -----------------------------------------------------------------------------
    // score() / score_topk() for B sequences at once.  Sequence b is ids[offsets[b], offsets[b + 1]) and its scored positions are
    // [firsts[b], len_b), 1 <= firsts[b] < len_b.  The outputs are flat, in sequence order then position order: logprob_out
    // [sum(len_b - firsts[b])], topk_ids_out / topk_logprob_out [sum, top_k] (top_k 1 .. KJARNI_SCORE_TOPK_MAX, <= vocab; slot 0 is
    // score()'s top / top_logprob); any output may be null.  score_plan_host (score_batch_kernels.h) packs the sequences into
    // chunks of at most 2 048 rows and computes a token prefix that neighbouring sequences share once (kScoreMinShared tokens or
    // more, never a scored token); every chunk runs embed_batch's layer stack once over its rows, the remainders of a group
    // attending to their prefix through launch_packed_prefix_attention, then only the rows whose successor is scored are
    // gathered through the final norm (launch_score_gather_norm) and reach the vocabulary head, score()'s score_head().  One
    // metadata upload and one result copy per chunk.  K and V live in the embed scratch: cache_len(), resident(), lanes, lookup
    // state, logits, last_hidden(), the prefix-reuse counters and score()'s buffers are left as they were.  Throws InvalidConfig
    // naming the argument and the sequence, before any GPU work, for non-monotone offsets, a sequence shorter than 2 or longer
    // than embed_max_tokens(), firsts[b] outside [1, len_b), an id >= vocab and top_k out of range; quantized checkpoints and
    // geometries forward() keeps off the matrix-core route are refused (GPT-2 is accepted).  B == 0 writes nothing.
    void score_batch(const uint32_t* ids, const int32_t* offsets, int B, const int32_t* firsts, int top_k, float* logprob_out,
                     uint32_t* topk_ids_out, float* topk_logprob_out);
    // Whether score_batch() takes this checkpoint (else it throws InvalidConfig, which says why).
    bool score_batch_supported() const;
    // The shortest shared prefix score_batch() computes once (the plan's min_shared).  Measured on the Llama-3.2-1B shape, 64 contexts
    // x 4 continuations of 16 tokens, a build with the constant at 1 (profiles/llm_score_batch_min_shared_1.jsonl): sharing a prefix of 1 / 4 / 16 / 64 / 256 tokens never
    // loses against the same shapes unshared (not shared / shared = 1.02 / 1.11 / 1.18 / 2.18 / 3.12), so length as such asks for
    // no floor.  But the plan's prefix only shrinks as neighbours join, and at 1 a neighbour that shares nothing but its first
    // token -- every sequence behind a BOS token -- joins a group of real sharers at q = 1 and takes its prefix down to 1: the
    // 64-token case behind a common first token then plans 20 235 rows in groups of prefix 1 instead of 8 192 in groups of prefix
    // 64, and 20 480 rows of those shapes measured 174.2 ms against 79.9 ms for the 8 192.  That one-token prefix loses against
    // not sharing it, hence 2; what 2 gives up is one row per member of a group that shares its first token only.
    static constexpr int kScoreMinShared = KJARNI_HIP_SCORE_MIN_SHARED;
    // Rows score_batch() computed / prefix rows it did not compute a second time (sum of (members - 1) * prefix), since load.
    uint64_t score_batch_rows() const { return score_batch_rows_; }
    uint64_t score_batch_saved_rows() const { return score_batch_saved_; }
    // ---- answer logits: a few chosen logits at the end of many sequences ------------------------------------------------------
    // logits_out[b, t] (row-major [B, n_targets]) = the logit of token targets[t] at the position after the last token of sequence
    // b = ids[offsets[b], offsets[b + 1]): dot(final_norm(h_last), head_row[targets[t]]), tied or untied head, f32 or bf16.  The
    // targets (1 .. kAnswerMaxTargets) are shared by the batch: 2 for a yes / no reranker, up to 8 for multiple choice by answer
    // letter.  answer_plan_host (score_batch_kernels.h) packs the sequences as score_batch does and computes a prefix that
    // neighbouring sequences share once, never with a sequence's last token in it; every chunk takes one metadata upload, runs
    // the packed layer stack, then launch_answer_logits over its sequences' last rows -- no vocabulary head -- and one copy of
    // its [n_seq, n_targets] logits.  K and V live in the embed scratch: cache_len(), resident(), lanes, lookup state, logits,
    // last_hidden(), the prefix-reuse counters and the buffers and counters of score() and score_batch() are left as they were.
    // Throws InvalidConfig naming the argument and the sequence, before any GPU work, for non-monotone offsets, a sequence
    // shorter than 2 or longer than embed_max_tokens(), an id or a target >= vocab and n_targets out of range; takes the
    // checkpoints score_batch() takes.  B == 0 writes nothing.
    void answer_logits_batch(const uint32_t* ids, const int32_t* offsets, int B, const uint32_t* targets, int n_targets, float* logits_out);
    // Rows answer_logits_batch() computed / prefix rows it did not compute a second time, since load (score_batch's pair is its own).
    uint64_t answer_rows() const { return answer_rows_; }
    uint64_t answer_saved_rows() const { return answer_saved_; }
    // Cache rows [first, first + rows) of one layer, K after RoPE (Qwen3: after the head norm and RoPE) and V, f32
    // [rows, kv_heads * head_dim] each (a test hook).
    void kv_rows(int layer, int first, int rows, float* k_out, float* v_out) const;
    void last_hidden(float* out, int rows) const;  // final-normed hidden states of the last (<= 8-row) pass
    void logits_to_host(float* out) const;
    uint32_t argmax();

    // run_generation_loop with the Greedy strategy: returns the generated ids (stop token excluded).
    std::vector<uint32_t> generate(const std::vector<uint32_t>& prompt, size_t max_new_tokens, float repetition_penalty,
                                   int no_repeat_ngram, const std::function<bool(uint32_t)>& on_token);
    // The same loop with a sampling strategy, explicit stop tokens and the max_length cap.
    // options.constraint (constraint_kernels.h: a byte DFA with its token mask on this model's device, over this model's
    // vocabulary): after every token the bytes of the emitted tokens are a prefix of a string the pattern matches; in an accepting
    // state the stop ids are legal.  Every step applies the mask before any logits processor and before the pick or the cut
    // (launch_constraint_apply), and the automaton's state lives on the device next to the token (launch_constraint_advance):
    // plain greedy replays pass -> apply -> argmax -> advance as one captured chain in the usual bursts and the host walks its own
    // copy of the DFA over the drained tokens; the device-sampling loop runs apply, the processors, then argmax or the cut; with
    // device sampling off the host masks its copy of the logits from the DFA and the token table.  A run also ends, without a stop
    // token, when the state is closed.  Throws InvalidConfig before any GPU work: a constraint of another device or vocabulary,
    // more than 16 stop ids, a state from which nothing can be emitted (DeviceConstraint::check_states).
    // options.grammar (grammar_kernels.h: a stack automaton in the DFA's place; both set is InvalidConfig): the same loop, with
    // "configuration" (state and stack) for "state", launch_grammar_apply / launch_grammar_advance for the two kernels, a third
    // captured chain for plain greedy, and DeviceGrammar::check_states for the refusal.
    // options.logprobs >= 0 with a sink (generation_run.h; logprob_kernels.h): one record per emitted token -- its log-probability
    // and the top_k most likely tokens under the log-softmax of the logits as the vocabulary head wrote them, before the mask, the
    // processors, temperature and the cut -- in every loop above: plain, constrained and grammar greedy replay chains of their own
    // with the slab pass and the record in them, the device-sampling loop runs the slab pass ahead of the mask and the processors
    // and the record once the host has decided, the host-sampling loop computes the record in float32 from the raw row.  The
    // prompt-lookup and draft-model loops are out of scope: generate_lookup, generate_lookup_sampled and generate_draft forward a
    // request that asks for records here (stats zero, the drafter untouched).  InvalidConfig before any GPU work for logprobs
    // outside -1 .. KJARNI_SCORE_TOPK_MAX or above the vocabulary.  generate_lanes / generate_wide take it per request.
    std::vector<uint32_t> generate(const std::vector<uint32_t>& prompt, const GenerateOptions& options,
                                   const std::function<bool(uint32_t)>& on_token);

    // ---- lanes: sequences decoded in lock step, each with its own KV cache and position.  Two banks of lanes share everything but
    // the step body: Bank::Lanes runs 1..kLanes sequences on the multi-row GEMV kernels, Bank::Wide 9..kWideLanes on the prompt GEMM.
    static constexpr int kLanes = 8;       // the GEMV kernels are built for <= 8 rows
    static constexpr int kWideLanes = 64;  // one M-tile of launch_prefill_gemm: every width up to it reads the weights once per step
    enum class Bank { Lanes, Wide };
    // generate() for every request, `lanes` (1..8, 0 = 8) of them at a time: the prompts are prefilled into lane caches of
    // min(context(), lane_context) rows (lane_context <= 0: context()) by the prompt routes of forward(), the live lanes then
    // step together (one captured graph per lane count for greedy requests without processors; requests with a repetition
    // penalty, an n-gram ban or sampling are decided lane by lane from that lane's logits row, uncaptured), and a lane that
    // finishes takes the next waiting request.  Returns one id vector per request, in request order: the ids generate() gives
    // for that request alone.  on_token(request, token) is called in step order, lane order within a step; false ends that
    // request only.  Throws InvalidConfig (before any GPU work) for lanes outside 0..8 or a prompt longer than a lane.
    std::vector<std::vector<uint32_t>> generate_lanes(const std::vector<LaneRequest>& requests, int lanes, int lane_context,
                                                      const std::function<bool(size_t, uint32_t)>& on_token);
    // Test hooks, one set for either bank: lane caches for `lanes` lanes (Lanes: 1..8, Wide: 9..64; 0 = the bank's most), all
    // empty; a prompt into one lane; one lock-step step over ids[lanes] for the lanes with live[lane] != 0 (the others are frozen:
    // nothing of theirs is read or written) returning the final-normed hidden rows [lanes, hidden] and logits [lanes, vocab]; a
    // lane's cache length and rows.
    void lanes_begin(Bank bank, int lanes, int lane_context);
    void lane_prefill(Bank bank, int lane, const uint32_t* ids, int n);
    // Test hook of the shared-prefix path: rows [0, s) of the single-sequence cache (s <= cache_len()) are copied into the lane
    // (one launch_kv_prefix_copy), then ids[0, n) are prefilled behind them; the lane holds s + n rows.
    void lane_prefill_shared(Bank bank, int lane, int s, const uint32_t* ids, int n);
    void lanes_step(Bank bank, const uint32_t* ids, const int32_t* live, float* hidden_out, float* logits_out);
    int lane_cache_len(Bank bank, int lane) const;
    int lane_capacity(Bank bank) const { return bank_of(bank).cap; }
    void lane_kv_rows(Bank bank, int lane, int layer, int first, int rows, float* k_out, float* v_out) const;
    // Projections of lane steps that took the multi-row weight-streaming kernel / fell back to the one-wave-per-column kernel
    // since load (counted when enqueued: a replayed graph counts once, at capture).
    uint64_t lane_stream_calls() const { return lane_stream_calls_; }
    uint64_t lane_fallback_calls() const { return lane_fallback_calls_; }

    // generate_lanes() for `lanes` (1..64, 0 = 64) requests at a time.  An effective width min(lanes, requests) of 8 or less runs
    // generate_lanes' own GEMV step; 9..64 runs the wide bank's step: the rows-route layer body (one Q|K|V GEMM into the lanes' staging
    // layout, rotate-and-scatter, the ragged decode attention, rows_finish()), the head as a GEMM, the wide pick -- captured once
    // per (width, lane capacity) for greedy requests without processors.  Results, callback order, stop rules, lane turnover,
    // prefix reuse and the processors / sampling path are generate_lanes'.  The lane caches cost 2 * layers * lanes * rows * kv
    // * 4 bytes with rows = min(context(), lane_context): 64 KB per token per lane on the Llama-1B shape (16 layers, kv 512),
    // 34 GB at 64 lanes of 8 192 rows -- set lane_context.  Throws InvalidConfig (before any GPU work) for lanes outside 0..64, an
    // empty prompt, a prompt longer than a lane, more than 16 stop ids, and -- above 8 lanes -- a quantized or FP8 checkpoint or a
    // geometry the rows route does not take.
    // Constrained requests (options.constraint or options.grammar, per request; generate_lanes takes them too): the lane that takes
    // the request gets the request's view and a fresh row in its slot of the device's lane automaton table (lane_constraint_kernels.h)
    // before its first pick.  Greedy requests without processors replay step -> (records' slab pass) -> lane apply -> pick -> lane
    // advance (-> records' finish) as one captured chain per (bank, width, records), and the host walks its own copy of each
    // request's automaton over the drained tokens, ending the request where generate() would; requests with processors or sampling
    // are decided lane by lane through the single-row launchers on the lane's slot, the mask ahead of the processors.  The ids and
    // the outcome (options.constraint_outcome) are generate()'s for that request alone.  A call whose requests carry no automaton
    // replays the plain chains: nothing of it changes.  InvalidConfig before any GPU work, naming the prompt: both set on one
    // request, an automaton of another device or vocabulary, more than 16 stop ids, check_states of that request's automaton.
    std::vector<std::vector<uint32_t>> generate_wide(const std::vector<LaneRequest>& requests, int lanes, int lane_context,
                                                     const std::function<bool(size_t, uint32_t)>& on_token = nullptr);

    // ---- prompt-lookup decoding: greedy generate() that emits several tokens per step ----------------------------------------
    // generate() for a greedy request without logits processors, with every step verifying a draft: the continuation of the
    // latest longest n-gram match in the prompt + the tokens so far (launch_lookup_draft) runs with the last token as one block
    // of draft_tokens + 1 rows at the device-held position (pass(), verify: causal inside the block, K / V rows into the cache,
    // every row through the final norm and the vocabulary head), and the pick keeps the model's own argmax tokens up to and
    // including the first one that differs from the draft.  Draft, step and pick are one chain of launches captured once per
    // row count and replayed in bursts (generate()'s cadences); near the end of the cache the steps have fewer rows, so that
    // nothing is written at or past the capacity.  Every emitted token is an argmax of the model's logits: the ids are
    // generate()'s wherever the two best logits are further apart than the float bar (the multi-row kernels sum in another
    // order).  A request that samples or has a processor runs generate() unchanged (stats stay zero).
    std::vector<uint32_t> generate_lookup(const std::vector<uint32_t>& prompt, const GenerateOptions& options, const LookupConfig& lookup,
                                          const std::function<bool(uint32_t)>& on_token, LookupStats* stats);
    // Test hook: one verify step on the cache as it stands: `token` and draft[n_draft] as rows 0..n_draft of a block of `rows`
    // rows (n_draft + 1 .. 8; the rows past the draft repeat its last id).  Returns the accepted length a; tokens_out[0..a] are
    // the picks, the cache grows by a + 1; logits_out (may be null) receives rows [0, n_draft] of the logits.
    int verify_step(uint32_t token, const uint32_t* draft, int n_draft, int rows, uint32_t* tokens_out, float* logits_out);
    // ---- prompt-lookup decoding for sampled requests ---------------------------------------------------------------------------
    // generate() for a request that samples (with or without a repetition penalty), several tokens per step.  Lookup drafts are
    // deterministic, so no rejection scheme is needed: generate() decides token i as a function of (processed logits, the i-th
    // draw); a verify step decides row 0 with the next draw, and while the result equals the draft the next row with the draw
    // after it; the first differing token is kept (lookup_accept_sampled, sampling.h).  Draws are taken one per decided row and
    // never for a row that is not reached, so the ids are generate()'s for the same draw stream and the stream is left where
    // generate() leaves it.  Per step one chain -- draft, verify pass, the rows penalty, the rows cut (captured once per row count
    // and filter arguments) -- then one copy and one synchronise; the host decides from each row's candidates and fetches a row's
    // processed logits only when they decline.  The a + 1 picks reach the device history, the token counts and the position in
    // one small upload ahead of the next step.  Greedy without processors forwards to generate_lookup; greedy with a penalty,
    // or any n-gram ban, to generate() (stats zero).
    std::vector<uint32_t> generate_lookup_sampled(const std::vector<uint32_t>& prompt, const GenerateOptions& options,
                                                  const LookupConfig& lookup, const std::function<bool(uint32_t)>& on_token,
                                                  LookupStats* stats);
    // Test hook: verify_step for a sampled request.  history[n_history]: the tokens the penalty counts, the last of them `token`
    // (not read when the penalty is 1); uniforms: one draw per decided row.  Returns a; picks_out[0..a]; *draws_used = a + 1;
    // logits_out (may be null) receives rows [0, n_draft] of the processed logits; the cache grows by a + 1.
    int verify_step_sampled(uint32_t token, const uint32_t* draft, int n_draft, int rows, const GenerateOptions& options,
                            const uint32_t* history, size_t n_history, const float* uniforms, uint32_t* picks_out, int* draws_used,
                            float* logits_out);
    // ---- speculative decoding with a draft model ---------------------------------------------------------------------------------
    // generate_lookup() / generate_lookup_sampled() with the draft of every verify step coming from `drafter`, a second model on
    // the same device with the same vocabulary and at least this model's context, instead of from the history.  One round on the
    // history T[0, n) (T[n - 1] in neither cache): launch_draft_begin puts the drafter at position n - 2 with the ids T[n - 2],
    // T[n - 1]; the drafter runs one 2-row pass (its argmax is draft 1) and rows - 2 single-row steps, each reading the id the
    // one before it handed over (launch_draft_handoff); then the target's verify pass and the pick (greedy) or the rows penalty
    // and the rows cut (sampled) run as in the lookup loops.  The drafter enqueues on this model's stream for the duration of the
    // call (StreamScope), so a round is one linear chain, captured once per (row count, drafter serial, options).  Re-running row
    // n - 2 keeps the launch shape fixed: after a round that accepted a of m drafts the drafter holds this model's rows, or one
    // fewer when a == m.  Every emitted token is this model's own decision: the ids are generate()'s (greedy: wherever the two
    // best logits are further apart than the float bar), whatever the drafter proposes.  Routing as generate_lookup_sampled:
    // greedy with a penalty, or any n-gram ban, runs generate() unchanged (stats zero, the drafter untouched).  Throws
    // InvalidConfig naming the argument, before any GPU work: drafter null / this model / on another device / another vocab / a
    // shorter context, draft_tokens outside 1..7, an empty or over-long prompt.  Afterwards the drafter's cache_len() is this
    // model's minus one (when a round ran) and its resident() the tokens of those rows.
    std::vector<uint32_t> generate_draft(LlmModel* drafter, const std::vector<uint32_t>& prompt, const GenerateOptions& options,
                                         int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats);
    // Test hook: one greedy round of `rows` (2..8) rows on the two caches as they stand, `token` being the token that is in
    // neither.  Needs resident() to cover this model's cache (>= 1 row) and the drafter to hold the same tokens up to
    // cache_len() - 1.  draft_out[rows - 1]: the drafter's proposals; returns a, tokens_out[0..a] the picks; logits_out (may be
    // null) receives the `rows` logits rows.  Both caches and resident lists advance as a loop's would.
    int draft_round(LlmModel* drafter, uint32_t token, int rows, uint32_t* draft_out, uint32_t* tokens_out, float* logits_out);
    // The refusals of generate_draft() that do not depend on the prompt.
    void check_draft_pair(const LlmModel* drafter, int draft_tokens) const;
    // Projections of verify steps that took the multi-row weight-streaming kernel / fell back (counted when enqueued).
    uint64_t verify_stream_calls() const { return verify_stream_calls_; }
    uint64_t verify_fallback_calls() const { return verify_fallback_calls_; }

private:
    LlmModel() = default;
    // Empties the cache down to the rows it may keep for `prompt` (all of them dropped with reuse off) and forwards the rest:
    // leaves the model as reset(); forward(prompt) does.
    void begin_sequence(const std::vector<uint32_t>& prompt);
    int keep_prefix(const uint32_t* prompt, size_t n, size_t limit);  // truncates the cache, counts; returns the rows kept
    void leave_resident(const std::vector<uint32_t>& all);            // what a generate loop leaves: the fed tokens of `all`
    // The record logs of a bank whose requests set logprobs: [lanes, hist stride] and [lanes, hist stride, KJARNI_SCORE_TOPK_MAX], a
    // slab scratch for all its rows and one raw-copy row, in one allocation of their own.
    struct LaneLogs {
        void* block = nullptr;
        int stride = 0;
        float *lp = nullptr, *tlp = nullptr, *copy = nullptr;
        uint32_t* ids = nullptr;
        void* scratch = nullptr;
    };
    // A bank of lock-step lanes: everything generate_on_lanes() and the test hooks need of one, allocated on first use.
    struct LaneBank {
        // the bank's constants: the step body it runs (lane_step() or wide_step_enqueue()), the widths it takes and their refusal,
        // the lanes of its state layout (LlmLaneState: 8, LlmWideState: 64) and that layout's size, what a step without a session says
        const bool wide;
        const int min_lanes, max_lanes;
        const char* const range_error;
        const int width;
        const size_t state_bytes;
        const char* const begin_error;
        LaneBank(bool wide_step, int lo, int hi, const char* range, int layout, size_t bytes, const char* begin)
            : wide(wide_step), min_lanes(lo), max_lanes(hi), range_error(range), width(layout), state_bytes(bytes), begin_error(begin)
        {
        }
        // per layer the lane-major caches [lanes][lane rows][kv] (one stride, alloc_cap * kv, addresses a lane)
        std::vector<float*> k, v;
        // One allocation of its own behind everything sized by lanes x rows or lanes x vocab, replaced when either grows: the
        // caches, the Q|K|V staging rows, the logits rows, the pick history [lanes, hist_stride], the logits processors' history,
        // distinct tokens, counts [lanes, vocab] and numbers of distinct tokens, and the wide bank's attention scratch.
        void* block = nullptr;
        int alloc = 0, alloc_cap = 0, lanes = 0, cap = 0, hist_stride = 0;  // allocated lanes x rows; the session's lanes x rows
        int len[kWideLanes] = {};                                          // the lanes' cache lengths
        float *qkv = nullptr, *logits = nullptr, *att = nullptr;
        int32_t *hist = nullptr, *ptok = nullptr, *pdistinct = nullptr;
        int *pcounts = nullptr, *pndistinct = nullptr;
        // fixed: the state on the device and its host mirror, each also by field, the pick scratch, and the device table of (main K,
        // lane-0 K, main V, lane-0 V) per layer that launch_kv_prefix_copy reads
        void* state = nullptr;
        std::unique_ptr<int32_t[]> mirror;
        LaneStateRef dev, host;
        unsigned long long* best = nullptr;
        LlmKvCopyPair* copy_table = nullptr;
        // captured chains by lane count: step -> pick; step -> records -> pick [k == 1 | k > 1]; step -> the automaton pick [no
        // records | k == 1 | k > 1]
        hipGraphExec_t graphs[kWideLanes + 1] = {}, lp_graphs[2][kWideLanes + 1] = {}, auto_graphs[3][kWideLanes + 1] = {};
        LaneLogs logs;
    };
    const LaneBank& bank_of(Bank b) const { return b == Bank::Wide ? wide_bank_ : lane_bank_; }
    LaneBank& bank_of(Bank b) { return b == Bank::Wide ? wide_bank_ : lane_bank_; }
    // Validates the width (the wide bank: also the checkpoint and the geometry its step takes), carves the block, builds the copy
    // table, and starts a session of `lanes` empty lanes.
    void ensure_lane_bank(LaneBank& b, int lanes, int lane_context);
    void drop_lane_record_graphs(LaneBank& b);  // the chains that hold the record logs or the automaton table
    void drop_lane_graphs(LaneBank& b);         // every captured chain of the bank
    void lane_state_to_device(LaneBank& b);
    void lane_state_from_device(LaneBank& b);
    void lane_copy_prefix(LaneBank& b, int lane, int s);  // rows [0, s) of every layer's K and V into the lane
    // A prompt into one lane behind `base` rows it already holds, through forward()'s routes: the layers' cache pointers (and the
    // capacity) are pointed at the lane for the call, the last position's logits become the lane's logits row.
    void lane_prefill_at(LaneBank& b, int lane, int base, const uint32_t* ids, int n);
    void lane_prefill_shared(LaneBank& b, int lane, int s, const uint32_t* ids, int n);
    // The two step bodies, each one lock-step step over lanes [0, lanes) of its bank enqueued on the stream, logits into the
    // bank's rows; lane_attention is the middle they share: rotate-and-scatter (Qwen3: behind the per-head norm) of the staging
    // rows into layer li's lane caches, then the ragged attention over `scratch` into `ctx`.
    void lane_step(int lanes);
    void wide_step_enqueue(int lanes);
    void lane_attention(const LaneBank& b, int lanes, size_t li, float* scratch, float* ctx);
    void lane_step_enqueue(LaneBank& b, int lanes);  // the bank's step body
    void lane_pick_enqueue(LaneBank& b, int lanes, int first, int advance);
    hipGraphExec_t lane_step_graph(LaneBank& b, int lanes);  // step + pick, captured once per (lane count, lane capacity)
    // `times` x (step + pick) replayed from the captured chain, or from `chain` in its place (the one with the records or the
    // automata in it)
    void lane_burst(LaneBank& b, int lanes, size_t times, hipGraphExec_t chain);
    // generate_lanes / generate_wide behind their own checks of `lanes`: n = min(lanes, requests) lanes of the bank.  strict: every
    // refusal is an InvalidConfig (generate_wide's contract).
    std::vector<std::vector<uint32_t>> generate_on_lanes(const std::vector<LaneRequest>& requests, int lanes, int lane_context,
                                                         const std::function<bool(size_t, uint32_t)>& on_token, LaneBank& b, bool strict);
    void* upload_weight(const std::vector<float>& host);  // f32 or bf16 according to bf16_
    float* upload_f32(const std::vector<float>& host);
    float* dalloc(size_t floats);
    void ensure_lookup();
    // Where the draft of a verify step comes from: the lookup rule on the history (drafter null), or a drafter model.
    struct DraftSource {
        LlmModel* drafter = nullptr;
        int ngram_max = 1, ngram_min = 1;  // the lookup rule's bounds (not read with a drafter)
        uint64_t serial() const { return drafter ? drafter->serial_ : 0; }
    };
    // For its lifetime `model` enqueues on `stream` instead of its own (which is synchronised first): how a drafter joins the
    // target's chain without a second stream or an event inside a capture.
    class StreamScope {
    public:
        StreamScope(LlmModel* model, hipStream_t stream);
        ~StreamScope();
        StreamScope(const StreamScope&) = delete;
        StreamScope& operator=(const StreamScope&) = delete;
    private:
        LlmModel* model_;
        hipStream_t saved_;
    };
    void enqueue_draft(int rows, const DraftSource& src);  // the ids of a verify block of `rows` rows into vids_, state->m
    void enqueue_verify(int rows, const DraftSource* src, bool record);  // [draft ->] step -> pick (src null: the ids are there)
    hipGraphExec_t lookup_graph(int rows, const DraftSource& src);
    std::vector<uint32_t> greedy_draft_loop(const std::vector<uint32_t>& prompt, const GenerateOptions& options, const DraftSource& src,
                                            int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats);
    std::vector<uint32_t> sampled_draft_loop(const std::vector<uint32_t>& prompt, const GenerateOptions& options, const DraftSource& src,
                                             int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats);
    void drafter_begin(const DraftSource& src, const std::vector<uint32_t>& prompt);  // the drafter's prompt rows (no-op without one)
    void drafter_leave(const DraftSource& src, const std::vector<uint32_t>& all, bool rounds_ran);
    void ensure_sampling();        // the device state of sampled decoding and the logits processors
    void ensure_lookup_sampled();
    // [draft ->] verify pass -> rows penalty -> rows cut over `src` rows of stride vocab (the verify logits, or logits_ for one row)
    void enqueue_verify_sampled(int rows, const DraftSource* src, const GenerateOptions& options);
    hipGraphExec_t lookup_sampled_graph(int rows, const DraftSource& src, const GenerateOptions& options);
    void rows_cut(float* logits, int rows, const GenerateOptions& options);  // rows penalty + rows cut + the copy (no sync)
    uint32_t decide_row(const float* logits_dev, int row, const GenerateOptions& options, float uniform);
    // One row's sampled token.  header (null: the cut was not attempted) and cand(i), candidate i of the row, are what the
    // step's copy brought to the host: the first `first` candidates; fetch_rest(n) brings the others of the n there are.  When the
    // candidates cannot decide, the row's processed logits come over from logits_dev and the full-array sampler runs.  Counts
    // the token in tokens_from_candidates_ / tokens_from_logits_; *decided (may be null): which of the two.
    template <class Cand, class FetchRest>
    uint32_t sample_row(const SampleHeader* header, int first, int capacity, Cand&& cand, FetchRest&& fetch_rest, const float* logits_dev,
                        const SamplingParams& params, float uniform, bool* decided);
    // "The history so far": the counts and the distinct list of tokens_dev[0, n), which `host` (may be null: they are there)
    // is uploaded to first.  Enqueued, not synchronised.
    void begin_token_history(int32_t* tokens_dev, const uint32_t* host, size_t n, int* counts, int32_t* distinct, int* ndistinct);
    void ensure_host_logits();  // the pinned row a logits fetch lands in
    void load_gpt2(SafeTensors& st, int weights);                      // GPT-2 tensors (Conv1D matrices transposed on the host)
    void finish_load();                                                // attention splits, workspace, stream
    // rows <= 8 through a quantized matrix; linear: a Q6_K matrix takes Q8_K activations (false: the tied head)
    void qlinear(const QMat& W, const float* X, int64_t ldx, int rows, bool linear, float* Y, int64_t ldy, const char* what);
    // n new tokens through the matrix-core GEMMs; score: each chunk's rows whose successor is scored go through the final norm
    // and score_head_rows
    // score_base: the position of ids[0] in the scored sequence (score() with a kept prefix forwards only the rest)
    void prefill_rows(const uint32_t* ids_host, int n, bool score = false, int score_base = 0);
    void ensure_prompt_workspace();  // the 2 048-row activation buffers of the prompt routes
    void ensure_packed_scratch();    // ek_, ev_, emeta_ and its pinned copy
    // The packed layer stack of embed_batch and score_batch over m rows of one chunk: embedding of ids_dev (GPT-2: + the learned
    // position row_pos[r]), then per layer rows_qkv() with K and V in ek_ / ev_, RoPE by row_pos, attention by the three block
    // tables, rows_finish().  Leaves the hidden states in ph_; the norm buffer pn_ is free afterwards.
    void packed_layers(int m, const uint32_t* ids_dev, const int32_t* row_pos, const EmbedBlock* vec, int n_vec, const EmbedBlock* mfma,
                       int n_mfma, const PrefixBlock* prefix, int n_prefix);
    // A packed chunk's metadata on the device: what upload_packed_meta() wrote, in its word order.
    struct PackedMeta {
        const uint32_t* ids;
        const int32_t *row_pos, *extra_a, *extra_b;
        const EmbedBlock *vec, *mfma;
        const PrefixBlock* prefix;
    };
    // ids [m] | row_pos [m] | extra_a [n_a] | extra_b [n_b] | vec | mfma | prefix into the pinned staging copy, then the chunk's one
    // upload.  Row r's id is ids[row_tok[r]], or ids[r] with row_tok null.  `entry` names the caller when the words exceed the buffer.
    PackedMeta upload_packed_meta(const char* entry, int m, const uint32_t* ids, const int32_t* row_tok, const int32_t* row_pos,
                                  const void* extra_a, size_t n_a, const void* extra_b, size_t n_b, const std::vector<EmbedBlock>& vec,
                                  const std::vector<EmbedBlock>& mfma, const std::vector<PrefixBlock>& prefix);
    // One projection of m prompt rows: Y[m, N] = A W^T (+ bias) (+ R), or with `gate`: gate = silu(gate) * (A W^T); gelu (GPT-2's
    // c_fc): Y = gelu_tanh(A W^T + bias).  Routes: the 64 x 64 prompt kernel, or from 512 rows and 208 tiles the 128 x 128-tile
    // GEMM (bf16 weights on the bf16 matrix cores); qm / fm: a GGUF-quantized / FP8 matrix, dequantized into the f32 scratch first.
    void prompt_proj(int m, const float* Ain, int lda, const void* W, const float* bias, const float* R, float* Y, int ldy, int N, int K,
                     float* gate, const char* what, const QMat* qm = nullptr, bool gelu = false, const Fp8Mat* fm = nullptr);
    void forward_rows(const uint32_t* ids, int n, bool score, int score_base = 0);  // forward(), with score()'s sink
    void ensure_score();
    void ensure_score_topk();
    void score_pass(const uint32_t* ids, int n, int first, int top_k);  // score() / score_topk() up to the copies
    // cnt final-normed rows Xn [cnt, hidden] of positions lo .. lo + cnt - 1 against the targets ids[lo + 1 ..]: their slots in
    // score()'s result rows, then score_head()
    void score_head_rows(const float* Xn, int lo, int cnt);
    // The vocabulary head of score(), score_topk() and score_batch() over cnt final-normed rows Xn [cnt, hidden] against tgt [cnt]:
    // the fused slab head where llm_score_head_takes (f32 / bf16 heads, unless set_score_fused(false)), else 8 rows at a time
    // through vlogits_ (quantized heads: qlinear) and the rows kernels; counted in score_fused_calls_ / score_rows_calls_.
    // k == 0: the plain kernels, ids / tlp [cnt] the arg-max and its log-probability; k >= 1: the top-k kernels, ids / tlp [cnt, k].
    void score_head(const float* Xn, int cnt, const uint32_t* tgt, int k, float* lp, uint32_t* ids, float* tlp);
    void enqueue_argmax(bool record);
    hipGraphExec_t step_graph();
    void ensure_constraint();                 // the model's descriptor, row state and state log
    hipGraphExec_t constrained_step_graph();  // pass -> apply -> argmax(record) -> advance, captured once (it reads cview_)
    void ensure_grammar();                    // the same for a grammar: descriptor, row state, state and depth logs
    hipGraphExec_t grammar_step_graph();      // pass -> grammar apply -> argmax(record) -> grammar advance (it reads gview_)
    // Generation log-probabilities (GenerateOptions::logprobs; logprob_kernels.h).  k is the width the device computes: 1 for a
    // request of 0 or 1 alternatives, else min(KJARNI_SCORE_TOPK_MAX, vocab) -- the host keeps the request's own top_k of them.
    void ensure_logprobs();                           // slab scratch, the raw copy of a row, the record logs beside hist_
    // The two launches over `rows` rows of `logits` [rows, vocab].  Finish: the chosen logit from `raw` (pitch vocab), the token at
    // token[row] (null: the row's arg-max), the record at index (count ? count[row] : 0) + bias of row `row`'s `stride` log entries.
    void logprob_partial_on(const float* logits, int rows, const int32_t* live, int k, void* scratch, float* copy);
    void logprob_finish_on(const float* logits, int rows, const int32_t* live, int k, void* scratch, const float* raw, const int32_t* token,
                           const int* count, int bias, int stride, float* lp, uint32_t* ids, float* tlp);
    // Lanes (generate_lanes / generate_wide with a request that sets logprobs): the bank's record logs; the two launches over
    // lanes [first, first + rows) ahead of the pick (frozen lanes write nothing; the record index is the lane's own device-held
    // count, so a lane that takes the next request starts at record 0); the captured chain step -> records -> pick.
    void ensure_lane_logprobs(LaneBank& b);
    void lane_logprobs_enqueue(LaneBank& b, int first, int rows, int k);
    hipGraphExec_t lane_logprob_step_graph(LaneBank& b, int lanes, int k);
    // Constrained lanes: the device's automaton table (allocated on first use) with its host copy; the pick of lanes [first, first
    // + rows) under their automata -- (records' slab pass) -> lane apply -> pick -> lane advance (-> records' finish, on the lanes
    // and tokens the advance reports) --; the captured chain step -> that, per (bank, lanes, no records | k == 1 | k > 1).
    void ensure_lane_automata();
    void lane_automaton_pick_enqueue(LaneBank& b, int first, int rows, int advance, bool records, int k);
    hipGraphExec_t lane_automaton_step_graph(LaneBank& b, int lanes, bool records, int k);
    void enqueue_logprob_partial(int k, bool copy);   // the slab pass over logits_ (copy: the row also goes to lp_copy_)
    // The record of the token at *token: read from lp_copy_ (from_copy) or logits_, written at index (count ? *count : 0) + bias.
    void enqueue_logprob_finish(int k, bool from_copy, const int32_t* token, const int* count, int bias);
    // The chains of plain greedy with records, captured once per (kind, k): kind 0 pass -> slab pass -> argmax(record) -> finish;
    // 1 / 2 pass -> slab pass (+ copy) -> constraint / grammar apply -> argmax(record) -> finish -> advance.
    hipGraphExec_t logprob_step_graph(int kind, int k);
    void fetch_logprobs(size_t first, size_t n, float* lp, uint32_t* ids, float* tlp);  // async copies of log rows [first, first + n)

    struct Layer {
        void *wqkv, *wo, *gate, *up, *down;  // GPT-2: c_attn, attn.c_proj, mlp.c_fc (in `gate`), mlp.c_proj (in `down`), as [out, in]
        float *bqkv, *ln1, *ln2;
        float *q_norm = nullptr, *k_norm = nullptr;  // Qwen3: per-head RMSNorm weights [head_dim]
        float *ln1_b = nullptr, *ln2_b = nullptr, *bo = nullptr, *bfc = nullptr, *bdown = nullptr;  // GPT-2's LayerNorm and projection biases
        float *k_cache, *v_cache;
        QMat q, k, v, o, gate_q, up_q, down_q;  // quantized checkpoints (wqkv ... down are then null)
        Fp8Mat fq, fk, fv, fo, fgate, fup, fdown;  // FP8 checkpoints (quant_ && fp8_): the codes and scales of the seven matrices
        // a sparse layer (qwen3_moe): the router [E, hidden] and the expert stacks [E, Im, hidden] x 2, [E, hidden, Im] in the weights'
        // dtype (gate / up / down are then null), and the record of the last pass: ids / weights [moe_rec_rows, k]
        bool moe = false;
        void *router = nullptr, *gate_stack = nullptr, *up_stack = nullptr, *down_stack = nullptr;
        int32_t* moe_ids = nullptr;
        float* moe_weights = nullptr;
        mutable int moe_rec_rows = 0;
    };
    // The sparse FFN behind the o-proj, h += MoE(RMSNorm(h)) (moe_kernels.h).  moe_steps: n <= 8 rows of h_, 4 launches;
    // moe_rows: m rows of ph_ in blocks of kMoeBlockRows rows (what bounds the slot-major scratch), 8 launches per block.
    static constexpr int kMoeBlockRows = 1024, kMoeRecordRows = 2048;
    void moe_steps(int n, const Layer& L);
    void moe_rows(int m, const Layer& L);
    // The layer body of the rows route, around the caller's own RoPE / head norm and attention (prefill_rows: the KV cache,
    // packed_layers: ek_ / ev_ and the block tables).  rows_qkv: norm 1 of ph_ into pn_, Q into pq_, K and V into the rows given.
    // rows_finish: o-proj of pctx_ + residual, norm 2, the SwiGLU or GPT-2 MLP, all into ph_.
    void rows_qkv(int m, const Layer& L, float* k_rows, float* v_rows);
    void rows_finish(int m, const Layer& L);
    // The steps route: passes of n <= 8 rows through the GEMV kernels, for every family.  Step: the decode step (n = 1, captured)
    // and prompt blocks; Verify: a block at the device-held position whose rows all reach the head; Lanes: one row per lane.
    enum class StepRoute { Step, Verify, Lanes };
    // One projection.  Step: launch_llm_gemv.  Verify / Lanes: launch_llm_gemv_lanes (the multi-row weight-streaming kernel where
    // it applies), counted in verify_stream_calls_ / verify_fallback_calls_ or lane_stream_calls_ / lane_fallback_calls_.
    void project(StepRoute route, const struct LlmGemvArgs& a, const char* what);
    // n new tokens at cache_len_ (device_pos: at *pos_): embedding, per layer step_qkv -> attention -> layer_finish, head.
    // verify: the one-row fusions are off and the final norm and the vocabulary head run over every row, into vlogits_ [n, vocab].
    void pass(const uint32_t* ids_dev, int n, bool device_pos, bool verify = false);
    // pass()'s first half of a layer: norm + Q|K|V + rotation, Q into q_, K and V into the cache rows at cache_len_ / *pos.
    // fused: the one-token Llama launch; embed_ids (non-null only with it, in the first layer): it gathers the embedding row too.
    void step_qkv(StepRoute route, int n, const Layer& L, const int* pos, bool fused, const uint32_t* embed_ids);
    // The second half, shared with lane_step(): o-proj + residual, norm + MLP-in (SwiGLU, or GPT-2's LayerNorm + c_fc + GELU-tanh),
    // down + residual, h_ -> h_.  slabs: the o-proj reads and merges the attention's split slabs in att_scratch_ instead of ctx_.
    // Quantized checkpoints: quant_finish().
    void layer_finish(StepRoute route, int n, const Layer& L, bool slabs);
    // The family branches every route shares.  embed_rows: n ids into dst (GPT-2 adds the learned position: pos + s, *pos_ptr + s,
    // or row_pos[s]).  final_norm: RMSNorm, GPT-2 LayerNorm.  head: rows normalised rows X into Y [rows, vocab]; norm_in_head (one
    // row, where llm_gemv_streams): X is the raw row, the head normalises it itself and stores it in last_.
    void embed_rows(const uint32_t* ids, int n, float* dst, int pos, const int* pos_ptr, const int* row_pos);
    void final_norm(const float* src, int rows, float* dst);
    void head(StepRoute route, const float* X, int rows, float* Y, bool norm_in_head = false);
    // The quantized stages over n <= 8 rows.  quant_source: the activation source of a stage, rows X (normalised by gamma inside
    // the GEMV), or -- when a Q6_K linear reads them -- one qprep launch writing the normalised rows and their Q8_K codes.
    // quant_finish (layer_finish's quantized form): o-proj + residual, RMSNorm + gate/up + SwiGLU, down + residual.
    void quant_source(QFusedArgs& a, int n, const float* X, int ldx, int k, const float* gamma, bool q8k, const char* what);
    void quant_finish(int n, const Layer& L);
    // FP8 checkpoints ride the quantized control flow with kernels of their own (fp8_kernels.hip).  fp8_qkv: norm + Q | K | V
    // as plain segments in one launch, Q into `q` (rows of ldq), K / V into rows row_off / *row_off_ptr + r of `kdst` / `vdst`.
    void fp8_qkv(int n, const Layer& L, float* q, int64_t ldq, float* kdst, float* vdst, int64_t ldkv, int row_off, const int* row_off_ptr);
    void fp8_finish(int n, const Layer& L);
    LlmConfig cfg_;
    int device_ = 0;
    uint64_t serial_ = 0;
    bool bf16_ = false, quant_ = false, gpt2_ = false;
    bool fp8_ = false;  // with quant_: the layers' matrices are FP8 codes; bf16_ then describes the embedding table and the head
    size_t weight_bytes_ = 0;
    uint64_t bytes_by_type_[32] = {};
    std::string config_json_;
    QMat qembed_, qhead_;       // quantized checkpoints: the table, and the head (== the table when tied)
    bool head_q8k_ = false;     // the head is a linear layer (untied output.weight), so a Q6_K head takes Q8_K activations
    float* xn_ = nullptr;       // quantized decode: normalised rows [8, max(H, I)]
    int8_t* xq_ = nullptr;      // their Q8_K codes
    float* xd_ = nullptr;       // and scales
    float* pact_ = nullptr;     // prompt route, Q6_K linears: the activation rows through Q8_K and back
    DeviceArena arena_;   // every device buffer of the model
    std::vector<Layer> layers_;
    void *embed_ = nullptr, *lm_head_ = nullptr;
    float *final_norm_ = nullptr, *cos_ = nullptr, *sin_ = nullptr;
    void* wpe_ = nullptr;               // GPT-2: learned position table [n_ctx, hidden], the weights' dtype
    float* final_norm_b_ = nullptr;     // GPT-2: ln_f bias
    // workspace
    float *h_ = nullptr, *q_ = nullptr, *ctx_ = nullptr, *mid_ = nullptr, *last_ = nullptr, *logits_ = nullptr, *att_scratch_ = nullptr;
    uint32_t* ids_ = nullptr;
    int32_t *token_ = nullptr, *hist_ = nullptr;
    int *pos_ = nullptr, *count_ = nullptr;
    unsigned long long* best_ = nullptr;
    int cache_len_ = 0, cache_cap_ = 0, last_rows_ = 0, hist_cap_ = 0, splits_ = 16;
    // prefill workspace (allocated on first use)
    float *moe_logits_ = nullptr, *moe_mid_ = nullptr;  // steps route: [8, E], [8 * k, Im]
    float *pmoe_logits_ = nullptr, *pmoe_mid_ = nullptr, *pmoe_y_ = nullptr;  // rows route: [block, E], [block * k, Im], [block * k, hidden]
    int32_t* pmoe_plan_ = nullptr;
    float *ph_ = nullptr, *pn_ = nullptr, *pq_ = nullptr, *pctx_ = nullptr, *pg_ = nullptr, *pu_ = nullptr;
    uint32_t* pids_ = nullptr;
    float* pw32_ = nullptr;    // f32 copy of the weight matrix a long prompt's GEMM is working on (bf16 checkpoints)
    float* psplit_ = nullptr;  // K-slice partial tiles of the prompt GEMMs (short prompts)
    // embed_batch (allocated on first use): a chunk's K and V rows [2048, kv], its ids | row positions | sequence starts | block
    // tables on the device and their pinned staging copy
    float *ek_ = nullptr, *ev_ = nullptr;
    int32_t *emeta_ = nullptr, *emeta_host_ = nullptr;
    // score_batch (allocated on first use): a chunk's results [logprob | top-k ids | top-k logprob], sized by the chunk's rows (a
    // chunk of many short sequences scores more rows than the context is long), and their pinned landing buffer
    uint32_t *sb_res_ = nullptr, *sb_res_host_ = nullptr;
    uint64_t score_batch_rows_ = 0, score_batch_saved_ = 0;
    uint64_t answer_rows_ = 0, answer_saved_ = 0;  // answer_logits_batch (its logits land in the norm buffer: no buffer of its own)
    float* host_logits_ = nullptr;  // pinned
    std::vector<uint32_t> row_ids_, row_cids_;  // sample_row's scratch: the distribution's ids, the candidates' ids
    std::vector<float> row_probs_, row_cvals_;  // ... and their probabilities / logits
    // sampled decoding on the device (allocated on first use): candidate header + list and its pinned mirror, the token
    // history with per-token counts and the list of distinct tokens (logits processors)
    static constexpr int kCandCap = 4096, kCandFirst = 512;
    void* samp_scratch_ = nullptr;
    uint8_t *samp_out_ = nullptr, *samp_host_ = nullptr;
    int32_t *samp_tokens_ = nullptr, *samp_distinct_ = nullptr;
    int *samp_counts_ = nullptr, *samp_ndistinct_ = nullptr;
    bool device_sampling_ = true;
    uint64_t tokens_from_candidates_ = 0, tokens_from_logits_ = 0;
    int prefill_cap_ = 0;
    uint64_t tile_gemm_calls_ = 0;
    hipStream_t stream_ = nullptr;
    hipGraphExec_t graph_ = nullptr;
    // constrained decoding (allocated on first use): the descriptor of the running call's constraint, its row state, the state
    // after every recorded pick (beside hist_), and the captured constrained step
    ConstraintView* cview_ = nullptr;
    ConstraintRow* crow_ = nullptr;
    uint32_t* cstate_log_ = nullptr;
    hipGraphExec_t cgraph_ = nullptr;
    // ... and under a grammar: the descriptor, the row (state, depth, stack), the state and depth logs, the captured chain
    GrammarView* gview_ = nullptr;
    GrammarRow* grow_ = nullptr;
    uint32_t* gstate_log_ = nullptr;
    int32_t* gdepth_log_ = nullptr;
    hipGraphExec_t ggraph_ = nullptr;
    // generation log-probabilities (allocated on first use): the slab scratch of one row, the raw copy of the row (taken before a
    // mask or a processor edits logits_), the token a host-decided step records, the record logs [hist_cap_] and [hist_cap_,
    // KJARNI_SCORE_TOPK_MAX] indexed as hist_, and the captured chains [plain | constrained | grammar][k == 1 | k > 1]
    void* lp_scratch_ = nullptr;
    float *lp_copy_ = nullptr, *lp_log_ = nullptr, *lp_tlp_log_ = nullptr;
    uint32_t* lp_ids_log_ = nullptr;
    int32_t* lp_tok_ = nullptr;
    hipGraphExec_t lp_graphs_[3][2] = {};
    LaneAutomatonTable* lane_auto_ = nullptr;
    std::unique_ptr<LaneAutomatonTable> lane_auto_host_;
    // the two banks of lanes (LaneBank above)
    LaneBank lane_bank_{false, 1, kLanes, "lanes must be 1..8", kMaxLanes, sizeof(LlmLaneState), "lanes_begin first"};
    LaneBank wide_bank_{true, kLanes + 1, kWideLanes, "wide lanes must be 9..64 (8 or fewer are the lanes route's)", kMaxWideLanes,
                        sizeof(LlmWideState), "wide_begin first"};
    uint64_t lane_stream_calls_ = 0, lane_fallback_calls_ = 0;
    // prompt-lookup decoding (allocated on first use): the ids and logits rows of a verify step, the device state, the history
    // (prompt + picks), the per-step (m, a) log, and one captured chain per row count for the n-gram bounds in lookup_ngram_
    float* vlogits_ = nullptr;
    uint32_t* vids_ = nullptr;
    LlmLookupState* lk_state_ = nullptr;
    int32_t *lk_hist_ = nullptr, *lk_log_ = nullptr;
    unsigned long long* lk_best_ = nullptr;
    int lk_hist_cap_ = 0;
    hipGraphExec_t lookup_graphs_[kLanes + 1] = {};
    int lookup_ngram_[2] = {0, 0};
    uint64_t lookup_serial_ = 0;  // the drafter the captured chains hold (0: the lookup rule)
    uint64_t verify_stream_calls_ = 0, verify_fallback_calls_ = 0;
    // sampled prompt-lookup (allocated on first use): per-row scratch, [8 headers | the rows' candidate slots in chunks of 512]
    // and its pinned mirror (a step copies the headers and the first chunk of its rows in one piece), the upload of a step's
    // picks, one captured chain per row count for the arguments in ls_args_
    static constexpr int kRowsCandCap = kCandCap;
    void* ls_scratch_ = nullptr;
    uint8_t *ls_out_ = nullptr, *ls_host_ = nullptr;
    int32_t *ls_up_ = nullptr, *ls_up_host_ = nullptr;
    uint32_t* ls_draft_host_ = nullptr;  // pinned: the ids of a step's verify block (a drafter's proposals, read back with the step's copy)
    hipGraphExec_t lookup_sampled_graphs_[kLanes + 1] = {};
    struct LookupSampledArgs {
        int ngram_max = 0, ngram_min = 0;
        uint64_t serial = 0;
        int64_t top_k = 0;
        float top_p = 0.0f, min_p = 0.0f, penalty = 0.0f;
    } ls_args_;
    // scoring (allocated on first use): the targets (ids shifted by one) and the three result rows [context], the slab
    // partials of the fused head; first_ / n_ of the call in flight
    uint32_t *score_tgt_ = nullptr, *score_top_ = nullptr;
    float *score_lp_ = nullptr, *score_tlp_ = nullptr;
    void* score_scratch_ = nullptr;
    size_t score_scratch_bytes_ = 0;
    int score_first_ = 0, score_n_ = 0;
    int score_k_ = 0;  // top_k of the running score_topk() call, 0 inside score()
    uint32_t* score_tk_ids_ = nullptr;  // [cache_cap_, KJARNI_SCORE_TOPK_MAX] each, used [n - first, top_k]
    float* score_tk_lp_ = nullptr;
    void* score_tk_scratch_ = nullptr;
    size_t score_tk_scratch_bytes_ = 0;
    bool score_fused_ = true;
    uint64_t score_fused_calls_ = 0, score_rows_calls_ = 0;
    // prefix reuse: the tokens of the cache rows (host only), the switch, the counters
    std::vector<uint32_t> resident_;
    bool prefix_reuse_ = false;
    bool fp8_mc_ = false;  // set_fp8_matrix_cores(): only ever true with fp8_
    uint64_t prefix_reused_ = 0, prefix_computed_ = 0;
};

}  // namespace kjarni
