// Token-level C ABI of the decoder-only path (kjarni_hip.h).  The reference's string-level chat group
// (crates/kjarni-ffi/src/chat.rs) sits on top of the same loop (crates/kjarni-transformers/src/decoder/
// generator.rs:228-381) plus a BPE tokenizer and chat templates, which are not built here.
#include <cstddef>
#include <cstring>
#include <fstream>
#include <iterator>
#include <mutex>

#include "decoder_embed_kernels.h"
#include "score_batch_kernels.h"
#include "answer_logits_kernels.h"
#include "llm_kernels.h"
#include "../../include/kjarni_hip.h"
#include "ffi_common.h"
#include "ffi_constraint.h"
#include "ffi_grammar.h"
#include "llm.h"
#include "fp8_weights.h"
#include "gguf.h"
#include "host_util.h"

using namespace kjarni;

struct KjarniHipDecoder {
    std::unique_ptr<LlmModel> model;
    mutable std::mutex mu;
};

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_load(const char* model_dir, int32_t device, int32_t weights_dtype, int32_t max_context,
                                                      KjarniHipDecoder** out)
{
    if (!model_dir || !out) return KJARNI_ERROR_NULL_POINTER;
    if (weights_dtype < 0 || weights_dtype > 2) return KJARNI_ERROR_INVALID_CONFIG;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        auto h = std::make_unique<KjarniHipDecoder>();
        h->model = LlmModel::load(model_dir, device, weights_dtype, max_context);
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_free(KjarniHipDecoder* d) { delete d; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_dims(const KjarniHipDecoder* d, int32_t* hidden, int32_t* layers, int32_t* vocab,
                                                      int32_t* context, int32_t* weights_bf16, uint64_t* weight_bytes)
{
    if (!d) return KJARNI_ERROR_NULL_POINTER;
    if (hidden) *hidden = d->model->config().hidden;
    if (layers) *layers = d->model->config().layers;
    if (vocab) *vocab = d->model->config().vocab;
    if (context) *context = d->model->context();
    if (weights_bf16) *weights_bf16 = d->model->bf16() ? 1 : 0;
    if (weight_bytes) *weight_bytes = (uint64_t)d->model->weight_bytes();
    return KJARNI_OK;
}

KJARNI_EXPORT uint64_t kjarni_hip_decoder_tile_gemm_calls(const KjarniHipDecoder* d) { return d ? d->model->tile_gemm_calls() : 0; }

KJARNI_EXPORT int32_t kjarni_hip_decoder_cache_len(const KjarniHipDecoder* d)
{
    if (!d) return 0;
    std::lock_guard<std::mutex> lock(d->mu);
    return d->model->cache_len();
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_kv_rows(const KjarniHipDecoder* d, int32_t layer, int32_t first, int32_t rows, float* k_out,
                                                         float* v_out)
{
    if (!d || !k_out || !v_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->kv_rows(layer, first, rows, k_out, v_out);  // range checked before anything is copied
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_moe_routing(KjarniHipDecoder* d, int32_t layer, int32_t rows_capacity, int32_t* rows,
                                                             int32_t* ids_out, float* weights_out)
{
    if (!d || !rows) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        const int n = d->model->moe_record_rows(layer);  // InvalidConfig for a dense layer or model, before anything is copied
        if (ids_out || weights_out) {
            if (!ids_out || !weights_out) throw InvalidConfig("ids_out and weights_out come together");
            if (rows_capacity < n) throw InvalidConfig("rows_capacity is below the " + std::to_string(n) + " rows recorded");
            d->model->moe_routing(layer, ids_out, weights_out);
        }
        *rows = n;
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_set_device_sampling(KjarniHipDecoder* d, int32_t on)
{
    if (d) d->model->set_device_sampling(on != 0);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_reset(KjarniHipDecoder* d)
{
    if (!d) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->reset();
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_forward(KjarniHipDecoder* d, const uint32_t* ids, int32_t n, float* hidden_out,
                                                         float* logits_out)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->forward(ids, n);
        if (hidden_out) d->model->last_hidden(hidden_out, n < 8 ? n : 8);
        if (logits_out) d->model->logits_to_host(logits_out);
    });
}

// The C callback as the loops take it (empty when there is none).  Token-level API: no tokenizer behind it, so no text.
static std::function<bool(uint32_t)> token_callback(KjarniTokenCallbackFn on_token, void* user_data)
{
    if (!on_token) return nullptr;
    return [on_token, user_data](uint32_t id) {
        KjarniToken t;
        t.text = nullptr;
        t.token_id = id;
        t.is_special = false;
        return on_token(t, user_data);
    };
}

static void copy_ids_out(const std::vector<uint32_t>& ids, uint32_t* ids_out, size_t capacity, size_t* n_out)
{
    *n_out = ids.size();
    if (capacity) std::memcpy(ids_out, ids.data(), std::min(capacity, ids.size()) * sizeof(uint32_t));
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate(KjarniHipDecoder* d, const uint32_t* prompt, size_t n_prompt,
                                                          size_t max_new_tokens, float repetition_penalty, int32_t no_repeat_ngram_size,
                                                          KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                          size_t capacity, size_t* n_out)
{
    if (!d || !prompt || !n_out || (capacity && !ids_out)) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        const std::vector<uint32_t> ids = d->model->generate(std::vector<uint32_t>(prompt, prompt + n_prompt), max_new_tokens,
                                                             repetition_penalty, no_repeat_ngram_size, cb);
        copy_ids_out(ids, ids_out, capacity, n_out);
    });
}

// ---- lanes: up to 8 prompts decoded in lock step -------------------------------------------------------------------------

// generate_batch and generate_wide: the same marshalling, the lanes route (1..8) or the wide entry (1..64)
static KjarniErrorCode generate_batch_on(KjarniHipDecoder* d, bool wide, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                         const size_t* max_new_tokens, float repetition_penalty, int32_t no_repeat_ngram_size, int32_t lanes,
                                         int32_t lane_context, KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                         size_t capacity, size_t* n_out, int32_t top_k = -1, float* logprob_out = nullptr,
                                         uint32_t* topk_ids_out = nullptr, float* topk_logprob_out = nullptr,
                                         const KjarniHipConstraint* const* constraints = nullptr,
                                         const KjarniHipGrammarConstraint* const* grammars = nullptr, KjarniHipLaneAutomatonResult* results = nullptr)
{
    if (!d) return KJARNI_ERROR_NULL_POINTER;
    if (n == 0) return KJARNI_OK;  // nothing to do, nothing written
    if (!offsets || !max_new_tokens || !n_out || (capacity && !ids_out) || (offsets[n] && !prompt_ids)) return KJARNI_ERROR_NULL_POINTER;
    for (size_t i = 0; i < n; ++i) n_out[i] = 0;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        if (wide && (lanes < 0 || lanes > LlmModel::kWideLanes)) throw InvalidConfig("lanes must be 0..64 (0 = 64)");
        if (!wide && (lanes < 0 || lanes > LlmModel::kLanes)) throw InvalidConfig("lanes must be 1..8 (0 = 8)");
        const int cap = lane_context <= 0 ? d->model->context() : std::min(d->model->context(), (int)lane_context);
        if (top_k < -1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > d->model->config().vocab)  // (-1: the entries without records)
            throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                                "] and not above the vocabulary (" + std::to_string(d->model->config().vocab) + ")");
        std::vector<LaneRequest> reqs(n);
        std::vector<TokenLogprobs> records(top_k >= 0 ? n : 0);
        std::vector<ConstraintOutcome> outcomes(constraints || grammars ? n : 0);
        for (size_t i = 0; i < n; ++i) {
            if (constraints && constraints[i]) reqs[i].options.constraint = constraints[i]->inner.get();
            if (grammars && grammars[i]) reqs[i].options.grammar = grammars[i]->inner.get();
            if (!outcomes.empty()) reqs[i].options.constraint_outcome = &outcomes[i];
            if (offsets[i + 1] < offsets[i]) throw InvalidConfig("prompt offsets must not decrease");
            if (wide && offsets[i + 1] == offsets[i]) throw InvalidConfig("cannot generate from empty prompt (prompt " + std::to_string(i) + ")");
            if (offsets[i + 1] - offsets[i] > (size_t)cap)  // before any GPU work
                throw InvalidConfig("prompt " + std::to_string(i) + " (" + std::to_string(offsets[i + 1] - offsets[i]) +
                                    " tokens) does not fit the lane capacity of " + std::to_string(cap) + " tokens");
            reqs[i].prompt.assign(prompt_ids + offsets[i], prompt_ids + offsets[i + 1]);
            reqs[i].options.max_new_tokens = max_new_tokens[i];
            reqs[i].options.repetition_penalty = repetition_penalty;
            reqs[i].options.no_repeat_ngram = no_repeat_ngram_size;
            if (top_k >= 0) {
                reqs[i].options.logprobs = top_k;
                reqs[i].options.logprob_sink = &records[i];
            }
        }
        std::function<bool(size_t, uint32_t)> cb;
        if (on_token)
            cb = [&](size_t prompt, uint32_t id) {
                KjarniToken t;
                t.text = nullptr;  // token-level API: no tokenizer behind it
                t.token_id = id;
                t.is_special = false;
                return on_token(prompt, t, user_data);
            };
        const std::vector<std::vector<uint32_t>> got =
            wide ? d->model->generate_wide(reqs, lanes, lane_context, cb) : d->model->generate_lanes(reqs, lanes, lane_context, cb);
        for (size_t i = 0; i < n; ++i) {
            n_out[i] = got[i].size();
            if (capacity) std::memcpy(ids_out + i * capacity, got[i].data(), std::min(capacity, got[i].size()) * sizeof(uint32_t));
            if (results) {
                const int32_t kind = reqs[i].options.constraint ? 1 : reqs[i].options.grammar ? 2 : 0;
                const ConstraintOutcome o = kind ? outcomes[i] : ConstraintOutcome();
                results[i] = KjarniHipLaneAutomatonResult{kind, o.final_state, o.device_state, o.final_depth, o.device_depth, o.accepted ? 1 : 0,
                                                          o.complete ? 1 : 0, o.violated ? 1 : 0};
            }
            if (top_k < 0) continue;
            const TokenLogprobs& r = records[i];
            if (r.logprob.size() != got[i].size()) throw std::runtime_error("generate: the records do not match the emitted tokens");
            const size_t m = std::min(capacity, got[i].size()), k = (size_t)top_k;
            if (logprob_out && m) std::memcpy(logprob_out + i * capacity, r.logprob.data(), m * sizeof(float));
            if (topk_ids_out && m && k) std::memcpy(topk_ids_out + i * capacity * k, r.topk_ids.data(), m * k * sizeof(uint32_t));
            if (topk_logprob_out && m && k) std::memcpy(topk_logprob_out + i * capacity * k, r.topk_logprob.data(), m * k * sizeof(float));
        }
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_batch(KjarniHipDecoder* d, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                                const size_t* max_new_tokens, float repetition_penalty,
                                                                int32_t no_repeat_ngram_size, int32_t lanes, int32_t lane_context,
                                                                KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                                size_t capacity, size_t* n_out)
{
    return generate_batch_on(d, false, prompt_ids, offsets, n, max_new_tokens, repetition_penalty, no_repeat_ngram_size, lanes, lane_context,
                             on_token, user_data, ids_out, capacity, n_out);
}

// ---- wide lanes: up to 64 prompts in lock step (LlmModel::generate_wide) ------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_wide(KjarniHipDecoder* d, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                               const size_t* max_new_tokens, float repetition_penalty,
                                                               int32_t no_repeat_ngram_size, int32_t lanes, int32_t lane_context,
                                                               KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                               size_t capacity, size_t* n_out)
{
    return generate_batch_on(d, true, prompt_ids, offsets, n, max_new_tokens, repetition_penalty, no_repeat_ngram_size, lanes, lane_context,
                             on_token, user_data, ids_out, capacity, n_out);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_wide_logprobs(KjarniHipDecoder* d, const uint32_t* prompt_ids, const size_t* offsets,
                                                                        size_t n, const size_t* max_new_tokens, float repetition_penalty,
                                                                        int32_t no_repeat_ngram_size, int32_t lanes, int32_t lane_context,
                                                                        KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                                        size_t capacity, size_t* n_out, int32_t top_k, float* logprob_out,
                                                                        uint32_t* topk_ids_out, float* topk_logprob_out)
{
    if (top_k < 0 || top_k > KJARNI_SCORE_TOPK_MAX) {  // (judged ahead of the handle)
        set_last_error("top_k (" + std::to_string(top_k) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) + "]");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    return generate_batch_on(d, true, prompt_ids, offsets, n, max_new_tokens, repetition_penalty, no_repeat_ngram_size, lanes, lane_context,
                             on_token, user_data, ids_out, capacity, n_out, top_k, logprob_out, topk_ids_out, topk_logprob_out);
}

// generate_wide_logprobs with an automaton per prompt (top_k = -1: no records)
KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_wide_constrained(KjarniHipDecoder* d, const uint32_t* prompt_ids, const size_t* offsets,
                                                                           size_t n, const size_t* max_new_tokens, float repetition_penalty,
                                                                           int32_t no_repeat_ngram_size, int32_t lanes, int32_t lane_context,
                                                                           KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                                           size_t capacity, size_t* n_out, int32_t top_k, float* logprob_out,
                                                                           uint32_t* topk_ids_out, float* topk_logprob_out,
                                                                           const KjarniHipConstraint* const* constraints,
                                                                           const KjarniHipGrammarConstraint* const* grammars,
                                                                           KjarniHipLaneAutomatonResult* results)
{
    if (top_k < -1 || top_k > KJARNI_SCORE_TOPK_MAX) {  // (judged ahead of the handle)
        set_last_error("top_k (" + std::to_string(top_k) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) + "] (-1: no records)");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    return generate_batch_on(d, true, prompt_ids, offsets, n, max_new_tokens, repetition_penalty, no_repeat_ngram_size, lanes, lane_context,
                             on_token, user_data, ids_out, capacity, n_out, top_k, logprob_out, topk_ids_out, topk_logprob_out, constraints, grammars,
                             results);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_wide_begin(KjarniHipDecoder* d, int32_t lanes, int32_t lane_context)
{
    if (!d) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        if (lanes != 0 && (lanes <= LlmModel::kLanes || lanes > LlmModel::kWideLanes))
            throw InvalidConfig("wide lanes must be 9..64 (0 = 64); 8 or fewer belong to lanes_begin");
        d->model->lanes_begin(LlmModel::Bank::Wide, lanes, lane_context);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_wide_prefill(KjarniHipDecoder* d, int32_t lane, const uint32_t* ids, int32_t n)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_prefill(LlmModel::Bank::Wide, lane, ids, n);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_wide_prefill_shared(KjarniHipDecoder* d, int32_t lane, int32_t shared, const uint32_t* ids,
                                                                     int32_t n)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_prefill_shared(LlmModel::Bank::Wide, lane, shared, ids, n);  // ranges checked before any GPU work
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_wide_step(KjarniHipDecoder* d, const uint32_t* ids, const int32_t* live, float* hidden_out,
                                                           float* logits_out)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lanes_step(LlmModel::Bank::Wide, ids, live, hidden_out, logits_out);
    });
}

KJARNI_EXPORT int32_t kjarni_hip_decoder_wide_cache_len(const KjarniHipDecoder* d, int32_t lane)
{
    if (!d) return -1;
    std::lock_guard<std::mutex> lock(d->mu);
    try {
        return d->model->lane_cache_len(LlmModel::Bank::Wide, lane);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

KJARNI_EXPORT int32_t kjarni_hip_decoder_wide_capacity(const KjarniHipDecoder* d)
{
    if (!d) return 0;
    std::lock_guard<std::mutex> lock(d->mu);
    return d->model->lane_capacity(LlmModel::Bank::Wide);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_wide_kv_rows(const KjarniHipDecoder* d, int32_t lane, int32_t layer, int32_t first, int32_t rows,
                                                              float* k_out, float* v_out)
{
    if (!d || !k_out || !v_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_kv_rows(LlmModel::Bank::Wide, lane, layer, first, rows, k_out, v_out);  // range checked before anything is copied
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_lanes_begin(KjarniHipDecoder* d, int32_t lanes, int32_t lane_context)
{
    if (!d) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        if (lanes < 0 || lanes > LlmModel::kLanes) throw InvalidConfig("lanes must be 1..8 (0 = 8)");
        d->model->lanes_begin(LlmModel::Bank::Lanes, lanes, lane_context);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_lane_prefill(KjarniHipDecoder* d, int32_t lane, const uint32_t* ids, int32_t n)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_prefill(LlmModel::Bank::Lanes, lane, ids, n);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_lanes_step(KjarniHipDecoder* d, const uint32_t* ids, const int32_t* live, float* hidden_out,
                                                            float* logits_out)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lanes_step(LlmModel::Bank::Lanes, ids, live, hidden_out, logits_out);
    });
}

KJARNI_EXPORT int32_t kjarni_hip_decoder_lane_cache_len(const KjarniHipDecoder* d, int32_t lane)
{
    if (!d) return -1;
    std::lock_guard<std::mutex> lock(d->mu);
    try {
        return d->model->lane_cache_len(LlmModel::Bank::Lanes, lane);
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return -1;
    }
}

KJARNI_EXPORT int32_t kjarni_hip_decoder_lane_capacity(const KjarniHipDecoder* d)
{
    if (!d) return 0;
    std::lock_guard<std::mutex> lock(d->mu);
    return d->model->lane_capacity(LlmModel::Bank::Lanes);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_lane_kv_rows(const KjarniHipDecoder* d, int32_t lane, int32_t layer, int32_t first, int32_t rows,
                                                              float* k_out, float* v_out)
{
    if (!d || !k_out || !v_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_kv_rows(LlmModel::Bank::Lanes, lane, layer, first, rows, k_out, v_out);  // range checked before anything is copied
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_lane_gemv_calls(const KjarniHipDecoder* d, uint64_t* streamed, uint64_t* fallback)
{
    if (streamed) *streamed = d ? d->model->lane_stream_calls() : 0;
    if (fallback) *fallback = d ? d->model->lane_fallback_calls() : 0;
}

// ---- prompt-lookup decoding ---------------------------------------------------------------------------------------------------

static LookupConfig lookup_config(const KjarniHipLookupConfig* c)  // NULL: the default; checked
{
    LookupConfig k;
    if (c) {
        k.draft_tokens = c->draft_tokens;
        k.ngram_max = c->ngram_max;
        k.ngram_min = c->ngram_min;
    }
    check_lookup_config(k);
    return k;
}

KJARNI_EXPORT KjarniHipLookupConfig kjarni_hip_lookup_config_default(void)
{
    const LookupConfig k;
    return KjarniHipLookupConfig{k.draft_tokens, k.ngram_max, k.ngram_min};
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_lookup(KjarniHipDecoder* d, const uint32_t* prompt, size_t n_prompt,
                                                                 size_t max_new_tokens, const uint32_t* stop_ids, size_t n_stop,
                                                                 const KjarniHipLookupConfig* config, KjarniTokenCallbackFn on_token,
                                                                 void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out,
                                                                 KjarniHipLookupStats* stats)
{
    if (!d || !prompt || !n_out || (capacity && !ids_out) || (n_stop && !stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const LookupConfig lk = lookup_config(config);
        std::lock_guard<std::mutex> lock(d->mu);
        if (n_prompt > (size_t)d->model->context())  // before any GPU work
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt;
        opt.max_new_tokens = max_new_tokens;
        opt.stop_ids.assign(stop_ids, stop_ids + n_stop);
        LookupStats st;
        const std::vector<uint32_t> ids = d->model->generate_lookup(std::vector<uint32_t>(prompt, prompt + n_prompt), opt, lk, cb, &st);
        copy_ids_out(ids, ids_out, capacity, n_out);
        if (stats) *stats = KjarniHipLookupStats{st.verify_steps, st.drafted_tokens, st.accepted_tokens, st.single_row_steps};
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_lookup_draft(const uint32_t* tokens, size_t n, const KjarniHipLookupConfig* config, uint32_t* draft_out,
                                                  int32_t* n_out)
{
    if ((n && !tokens) || !draft_out || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        const std::vector<uint32_t> draft = lookup_draft_host(tokens, n, lookup_config(config));
        std::memcpy(draft_out, draft.data(), draft.size() * sizeof(uint32_t));
        *n_out = (int32_t)draft.size();
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_verify_step(KjarniHipDecoder* d, uint32_t token, const uint32_t* draft, int32_t n_draft,
                                                             int32_t rows, uint32_t* tokens_out, int32_t* n_accepted, float* logits_out)
{
    if (!d || !tokens_out || !n_accepted || (n_draft > 0 && !draft)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        *n_accepted = d->model->verify_step(token, draft, n_draft, rows, tokens_out, logits_out);  // ranges checked before any GPU work
    });
}

// ---- prompt-lookup decoding for sampled requests ------------------------------------------------------------------------------

static GenerateOptions sampling_options(const KjarniHipSamplingOptions& o)
{
    GenerateOptions g;
    g.max_new_tokens = o.max_new_tokens;
    g.repetition_penalty = o.repetition_penalty;
    g.no_repeat_ngram = o.no_repeat_ngram;
    g.sample = o.sample != 0;
    g.sampling.temperature = o.temperature;
    g.sampling.top_k = o.top_k;
    g.sampling.top_p = o.top_p;
    g.sampling.min_p = o.min_p;
    if (o.n_stop) g.stop_ids.assign(o.stop_ids, o.stop_ids + o.n_stop);
    return g;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_sampled(KjarniHipDecoder* d, const uint32_t* prompt, size_t n_prompt,
                                                                  const KjarniHipSamplingOptions* options, const KjarniHipLookupConfig* lookup,
                                                                  KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                                  size_t capacity, size_t* n_out, KjarniHipLookupStats* stats)
{
    if (!options || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    if (options->uniforms && options->n_uniforms < options->max_new_tokens) {  // (the options are judged on their own, ahead of the handle)
        set_last_error("n_uniforms (" + std::to_string(options->n_uniforms) + ") is less than max_new_tokens (" +
                       std::to_string(options->max_new_tokens) + ")");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (!d || (n_prompt && !prompt) || (capacity && !ids_out) || (options->n_stop && !options->stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // everything that can be refused is refused before any GPU work
        LookupConfig lk;
        if (lookup) lk = lookup_config(lookup);
        if (n_prompt == 0) throw InvalidConfig("cannot generate from an empty prompt");
        std::lock_guard<std::mutex> lock(d->mu);
        if (n_prompt > (size_t)d->model->context())
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt = sampling_options(*options);
        UniformRng rng(options->seed);
        size_t drawn = 0;
        const float* u = options->uniforms;
        const size_t n_u = options->n_uniforms;
        if (u)  // one draw per decided token, never more than max_new_tokens of them: a loop that asks for more has gone wrong
            opt.uniform = [&drawn, u, n_u] {
                if (drawn >= n_u) throw std::runtime_error("the draw stream is exhausted: more draws than uniforms");
                return u[drawn++];
            };
        else opt.uniform = [&rng] { return rng.next(); };
        const std::vector<uint32_t> p(prompt, prompt + n_prompt);
        LookupStats st;
        const std::vector<uint32_t> ids = lookup ? d->model->generate_lookup_sampled(p, opt, lk, cb, &st) : d->model->generate(p, opt, cb);
        copy_ids_out(ids, ids_out, capacity, n_out);
        if (stats) *stats = KjarniHipLookupStats{st.verify_steps, st.drafted_tokens, st.accepted_tokens, st.single_row_steps};
    });
}

// ---- constrained decoding --------------------------------------------------------------------------------------------------------

// kjarni_hip_decoder_generate_sampled's plain loop with options.constraint set; the draws as there.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_constrained(KjarniHipDecoder* d, const KjarniHipConstraint* constraint,
                                                                      const uint32_t* prompt, size_t n_prompt,
                                                                      const KjarniHipSamplingOptions* options, KjarniTokenCallbackFn on_token,
                                                                      void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out,
                                                                      KjarniHipConstraintResult* result)
{
    if (!options || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    if (result) *result = KjarniHipConstraintResult{};
    if (options->uniforms && options->n_uniforms < options->max_new_tokens) {  // (the options are judged on their own, ahead of the handles)
        set_last_error("n_uniforms (" + std::to_string(options->n_uniforms) + ") is less than max_new_tokens (" +
                       std::to_string(options->max_new_tokens) + ")");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (!d || !constraint || (n_prompt && !prompt) || (capacity && !ids_out) || (options->n_stop && !options->stop_ids))
        return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_prompt == 0) throw InvalidConfig("cannot generate from an empty prompt");
        std::lock_guard<std::mutex> lock(d->mu);
        if (n_prompt > (size_t)d->model->context())
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt = sampling_options(*options);
        UniformRng rng(options->seed);
        size_t drawn = 0;
        const float* u = options->uniforms;
        const size_t n_u = options->n_uniforms;
        if (u)
            opt.uniform = [&drawn, u, n_u] {
                if (drawn >= n_u) throw std::runtime_error("the draw stream is exhausted: more draws than uniforms");
                return u[drawn++];
            };
        else opt.uniform = [&rng] { return rng.next(); };
        ConstraintOutcome outcome;
        opt.constraint = constraint->inner.get();
        opt.constraint_outcome = &outcome;
        const std::vector<uint32_t> ids = d->model->generate(std::vector<uint32_t>(prompt, prompt + n_prompt), opt, cb);  // refusals first
        copy_ids_out(ids, ids_out, capacity, n_out);
        if (result)
            *result = KjarniHipConstraintResult{outcome.final_state, outcome.device_state, outcome.accepted ? 1 : 0, outcome.complete ? 1 : 0,
                                                outcome.violated ? 1 : 0};
    });
}

// kjarni_hip_decoder_generate_constrained with a grammar in the constraint's place (options.grammar): the same loop, the draws as there.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_grammar(KjarniHipDecoder* d, const KjarniHipGrammarConstraint* grammar, const uint32_t* prompt,
                                                                  size_t n_prompt, const KjarniHipSamplingOptions* options,
                                                                  KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out, size_t capacity,
                                                                  size_t* n_out, KjarniHipGrammarResult* result)
{
    if (!options || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    if (result) *result = KjarniHipGrammarResult{};
    if (options->uniforms && options->n_uniforms < options->max_new_tokens) {  // (the options are judged on their own, ahead of the handles)
        set_last_error("n_uniforms (" + std::to_string(options->n_uniforms) + ") is less than max_new_tokens (" +
                       std::to_string(options->max_new_tokens) + ")");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (!d || !grammar || (n_prompt && !prompt) || (capacity && !ids_out) || (options->n_stop && !options->stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_prompt == 0) throw InvalidConfig("cannot generate from an empty prompt");
        std::lock_guard<std::mutex> lock(d->mu);
        if (n_prompt > (size_t)d->model->context())
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt = sampling_options(*options);
        UniformRng rng(options->seed);
        size_t drawn = 0;
        const float* u = options->uniforms;
        const size_t n_u = options->n_uniforms;
        if (u)
            opt.uniform = [&drawn, u, n_u] {
                if (drawn >= n_u) throw std::runtime_error("the draw stream is exhausted: more draws than uniforms");
                return u[drawn++];
            };
        else opt.uniform = [&rng] { return rng.next(); };
        ConstraintOutcome outcome;
        opt.grammar = grammar->inner.get();
        opt.constraint_outcome = &outcome;
        const std::vector<uint32_t> ids = d->model->generate(std::vector<uint32_t>(prompt, prompt + n_prompt), opt, cb);  // refusals first
        copy_ids_out(ids, ids_out, capacity, n_out);
        if (result)
            *result = KjarniHipGrammarResult{outcome.final_state, outcome.device_state, outcome.final_depth, outcome.device_depth,
                                             outcome.accepted ? 1 : 0, outcome.complete ? 1 : 0, outcome.violated ? 1 : 0};
    });
}

// ---- generation log-probabilities ------------------------------------------------------------------------------------------------

// The plain loop of the three entries above (constraint / grammar: at most one, either may be NULL) with options.logprobs set;
// the draws as there.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_logprobs(KjarniHipDecoder* d, const KjarniHipConstraint* constraint,
                                                                   const KjarniHipGrammarConstraint* grammar, const uint32_t* prompt, size_t n_prompt,
                                                                   const KjarniHipSamplingOptions* options, int32_t top_k,
                                                                   KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                                   size_t capacity, size_t* n_out, float* logprob_out, uint32_t* topk_ids_out,
                                                                   float* topk_logprob_out, KjarniHipConstraintResult* constraint_result,
                                                                   KjarniHipGrammarResult* grammar_result)
{
    if (!options || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    if (constraint_result) *constraint_result = KjarniHipConstraintResult{};
    if (grammar_result) *grammar_result = KjarniHipGrammarResult{};
    if (options->uniforms && options->n_uniforms < options->max_new_tokens) {  // (the options are judged on their own, ahead of the handles)
        set_last_error("n_uniforms (" + std::to_string(options->n_uniforms) + ") is less than max_new_tokens (" +
                       std::to_string(options->max_new_tokens) + ")");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (top_k < 0 || top_k > KJARNI_SCORE_TOPK_MAX) {
        set_last_error("top_k (" + std::to_string(top_k) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) + "]");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (constraint && grammar) {
        set_last_error("a call takes a constraint or a grammar, not both");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (!d || (n_prompt && !prompt) || (capacity && !ids_out) || (options->n_stop && !options->stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_prompt == 0) throw InvalidConfig("cannot generate from an empty prompt");
        std::lock_guard<std::mutex> lock(d->mu);
        if (n_prompt > (size_t)d->model->context())
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt = sampling_options(*options);
        UniformRng rng(options->seed);
        size_t drawn = 0;
        const float* u = options->uniforms;
        const size_t n_u = options->n_uniforms;
        if (u)
            opt.uniform = [&drawn, u, n_u] {
                if (drawn >= n_u) throw std::runtime_error("the draw stream is exhausted: more draws than uniforms");
                return u[drawn++];
            };
        else opt.uniform = [&rng] { return rng.next(); };
        ConstraintOutcome outcome;
        if (constraint) opt.constraint = constraint->inner.get();
        if (grammar) opt.grammar = grammar->inner.get();
        opt.constraint_outcome = &outcome;
        TokenLogprobs records;
        opt.logprobs = top_k;
        opt.logprob_sink = &records;
        const std::vector<uint32_t> ids = d->model->generate(std::vector<uint32_t>(prompt, prompt + n_prompt), opt, cb);  // refusals first
        copy_ids_out(ids, ids_out, capacity, n_out);
        const size_t n = std::min(std::min(ids.size(), capacity), records.logprob.size());
        if (logprob_out && n) std::memcpy(logprob_out, records.logprob.data(), n * sizeof(float));
        if (topk_ids_out && n && top_k) std::memcpy(topk_ids_out, records.topk_ids.data(), n * (size_t)top_k * sizeof(uint32_t));
        if (topk_logprob_out && n && top_k) std::memcpy(topk_logprob_out, records.topk_logprob.data(), n * (size_t)top_k * sizeof(float));
        if (records.logprob.size() != ids.size()) throw std::runtime_error("generate: the records do not match the emitted tokens");
        if (constraint && constraint_result)
            *constraint_result = KjarniHipConstraintResult{outcome.final_state, outcome.device_state, outcome.accepted ? 1 : 0,
                                                           outcome.complete ? 1 : 0, outcome.violated ? 1 : 0};
        if (grammar && grammar_result)
            *grammar_result = KjarniHipGrammarResult{outcome.final_state, outcome.device_state, outcome.final_depth, outcome.device_depth,
                                                     outcome.accepted ? 1 : 0, outcome.complete ? 1 : 0, outcome.violated ? 1 : 0};
    });
}

// ---- speculative decoding with a draft model -----------------------------------------------------------------------------------

// Both handles' locks, in address order (two calls with the handles swapped cannot deadlock); draft == d is refused before.
struct DraftPairLock {
    std::unique_lock<std::mutex> first, second;
    DraftPairLock(KjarniHipDecoder* a, KjarniHipDecoder* b)
    {
        if (b < a) std::swap(a, b);
        first = std::unique_lock<std::mutex>(a->mu);
        second = std::unique_lock<std::mutex>(b->mu);
    }
};

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_generate_draft(KjarniHipDecoder* d, KjarniHipDecoder* draft, const uint32_t* prompt,
                                                                size_t n_prompt, const KjarniHipSamplingOptions* options,
                                                                int32_t draft_tokens, KjarniTokenCallbackFn on_token, void* user_data,
                                                                uint32_t* ids_out, size_t capacity, size_t* n_out,
                                                                KjarniHipLookupStats* stats)
{
    if (!options || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    if (options->uniforms && options->n_uniforms < options->max_new_tokens) {
        set_last_error("n_uniforms (" + std::to_string(options->n_uniforms) + ") is less than max_new_tokens (" +
                       std::to_string(options->max_new_tokens) + ")");
        return KJARNI_ERROR_INVALID_CONFIG;
    }
    if (!d || (n_prompt && !prompt) || (capacity && !ids_out) || (options->n_stop && !options->stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // everything that can be refused is refused before any GPU work
        if (!draft) throw InvalidConfig("draft must not be null");
        if (draft == d) throw InvalidConfig("draft must be another model than the decoder itself");
        DraftPairLock lock(d, draft);
        d->model->check_draft_pair(draft->model.get(), draft_tokens);
        if (n_prompt == 0) throw InvalidConfig("prompt must not be empty");
        if (n_prompt > (size_t)d->model->context())
            throw InvalidConfig("prompt (" + std::to_string(n_prompt) + " tokens) does not fit the context of " +
                                std::to_string(d->model->context()) + " tokens");
        const std::function<bool(uint32_t)> cb = token_callback(on_token, user_data);
        GenerateOptions opt = sampling_options(*options);
        UniformRng rng(options->seed);
        size_t drawn = 0;
        const float* u = options->uniforms;
        const size_t n_u = options->n_uniforms;
        if (u)
            opt.uniform = [&drawn, u, n_u] {
                if (drawn >= n_u) throw std::runtime_error("the draw stream is exhausted: more draws than uniforms");
                return u[drawn++];
            };
        else opt.uniform = [&rng] { return rng.next(); };
        LookupStats st;
        const std::vector<uint32_t> ids =
            d->model->generate_draft(draft->model.get(), std::vector<uint32_t>(prompt, prompt + n_prompt), opt, draft_tokens, cb, &st);
        copy_ids_out(ids, ids_out, capacity, n_out);
        if (stats) *stats = KjarniHipLookupStats{st.verify_steps, st.drafted_tokens, st.accepted_tokens, st.single_row_steps};
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_draft_round(KjarniHipDecoder* d, KjarniHipDecoder* draft, uint32_t token, int32_t rows,
                                                             uint32_t* draft_out, uint32_t* tokens_out, int32_t* n_accepted,
                                                             float* logits_out)
{
    if (!d || !draft_out || !tokens_out || !n_accepted) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (!draft) throw InvalidConfig("draft must not be null");
        if (draft == d) throw InvalidConfig("draft must be another model than the decoder itself");
        DraftPairLock lock(d, draft);
        *n_accepted = d->model->draft_round(draft->model.get(), token, rows, draft_out, tokens_out, logits_out);  // checked before any GPU work
    });
}

KJARNI_EXPORT size_t kjarni_hip_sampling_options_layout(size_t* out, size_t capacity)
{
    using O = KjarniHipSamplingOptions;
    const size_t v[] = {sizeof(O), offsetof(O, max_new_tokens), offsetof(O, repetition_penalty), offsetof(O, no_repeat_ngram),
                        offsetof(O, sample), offsetof(O, temperature), offsetof(O, top_k), offsetof(O, top_p), offsetof(O, min_p),
                        offsetof(O, stop_ids), offsetof(O, n_stop), offsetof(O, uniforms), offsetof(O, n_uniforms), offsetof(O, seed)};
    const size_t n = sizeof(v) / sizeof(v[0]);
    for (size_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
    return n;
}

KJARNI_EXPORT void kjarni_hip_decoder_sampling_routes(const KjarniHipDecoder* d, uint64_t* from_candidates, uint64_t* from_logits)
{
    if (from_candidates) *from_candidates = d ? d->model->tokens_from_candidates() : 0;
    if (from_logits) *from_logits = d ? d->model->tokens_from_logits() : 0;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_verify_step_sampled(KjarniHipDecoder* d, uint32_t token, const uint32_t* draft, int32_t n_draft,
                                                                     int32_t rows, const KjarniHipSamplingOptions* options,
                                                                     const uint32_t* history, size_t n_history, const float* uniforms,
                                                                     uint32_t* picks_out, int32_t* accepted_out, int32_t* draws_used_out,
                                                                     float* logits_out)
{
    if (!d || !options || !uniforms || !picks_out || !accepted_out || (n_draft > 0 && !draft) || (n_history && !history))
        return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        int used = 0;
        *accepted_out = d->model->verify_step_sampled(token, draft, n_draft, rows, sampling_options(*options), history, n_history, uniforms, picks_out, &used,
                                                      logits_out);  // ranges checked before any GPU work
        if (draws_used_out) *draws_used_out = used;
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_lookup_accept_sampled(const float* logits, int64_t ld, int32_t rows, size_t vocab, const uint32_t* draft,
                                                           int32_t n_draft, float temperature, int64_t top_k, float top_p, float min_p,
                                                           const float* uniforms, uint32_t* picks_out, int32_t* accepted_out,
                                                           int32_t* draws_used_out)
{
    if (!logits || !uniforms || !picks_out || !accepted_out || (n_draft > 0 && !draft)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        if (rows < 1 || rows > LlmModel::kLanes || n_draft < 0 || vocab < 1 || ld < (int64_t)vocab)
            throw InvalidConfig("invalid block (rows 1..8, n_draft >= 0, vocab >= 1, ld >= vocab)");
        SamplingParams p;
        p.temperature = temperature;
        p.top_k = top_k;
        p.top_p = top_p;
        p.min_p = min_p;
        int used = 0;
        *accepted_out = lookup_accept_sampled(logits, ld, rows, vocab, draft, n_draft, p, [&] { return uniforms[used++]; }, picks_out);
        if (draws_used_out) *draws_used_out = used;
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_verify_gemv_calls(const KjarniHipDecoder* d, uint64_t* streamed, uint64_t* fallback)
{
    if (streamed) *streamed = d ? d->model->verify_stream_calls() : 0;
    if (fallback) *fallback = d ? d->model->verify_fallback_calls() : 0;
}

// ---- scoring ---------------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_score(KjarniHipDecoder* d, const uint32_t* ids, int32_t n, int32_t first, float* logprob_out,
                                                       uint32_t* top_out, float* top_logprob_out)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->score(ids, n, first, logprob_out, top_out, top_logprob_out);  // arguments checked before any GPU work
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_score_topk(KjarniHipDecoder* d, const uint32_t* ids, int32_t n, int32_t first, int32_t top_k,
                                                            float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->score_topk(ids, n, first, top_k, logprob_out, topk_ids_out, topk_logprob_out);  // arguments checked before any GPU work
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_set_score_fused(KjarniHipDecoder* d, int32_t on)
{
    if (d) d->model->set_score_fused(on != 0);
}

KJARNI_EXPORT void kjarni_hip_decoder_score_calls(const KjarniHipDecoder* d, uint64_t* fused, uint64_t* rows)
{
    if (fused) *fused = d ? d->model->score_fused_calls() : 0;
    if (rows) *rows = d ? d->model->score_rows_calls() : 0;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_score_batch(KjarniHipDecoder* d, const uint32_t* ids, const int32_t* offsets,
                                                             int32_t n_sequences, const int32_t* firsts, int32_t top_k, float* logprob_out,
                                                             uint32_t* topk_ids_out, float* topk_logprob_out)
{
    if (!d || (n_sequences > 0 && (!ids || !offsets || !firsts))) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->score_batch(ids, offsets, n_sequences, firsts, top_k, logprob_out, topk_ids_out, topk_logprob_out);  // checked before any GPU work
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_score_batch_rows(const KjarniHipDecoder* d, uint64_t* computed, uint64_t* saved)
{
    if (computed) *computed = d ? d->model->score_batch_rows() : 0;
    if (saved) *saved = d ? d->model->score_batch_saved_rows() : 0;
}

namespace {

// The chunks, the groups and the three block tables of a plan into the caller's arrays (kjarni_hip_score_plan and
// kjarni_hip_answer_plan share them; the gather table is each one's own).  Tables may be null; the counts are always written.
void put_plan_tables(const ScorePlan& plan, int32_t n, int32_t* chunk_first_seq, int32_t* chunk_rows, int32_t* n_chunks, int32_t* groups,
                     int32_t group_capacity, int32_t* n_groups, int32_t* vec_blocks, int32_t vec_capacity, int32_t* n_vec, int32_t* mfma_blocks,
                     int32_t mfma_capacity, int32_t* n_mfma, int32_t* prefix_blocks, int32_t prefix_capacity, int32_t* n_prefix)
{
    int32_t nv = 0, nm = 0, np = 0;
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const ScoreChunk& ch = plan.chunks[c];
        if (chunk_first_seq) chunk_first_seq[c] = ch.first_seq;
        if (chunk_rows) chunk_rows[c] = ch.rows;
        auto put = [&](const std::vector<EmbedBlock>& src, int32_t* dst, int32_t cap, int32_t& cnt) {
            for (const EmbedBlock& b : src) {
                if (dst && cnt < cap) {
                    int32_t* w = dst + 4 * (size_t)cnt;
                    w[0] = (int32_t)c; w[1] = b.first; w[2] = b.q0; w[3] = b.len;
                }
                ++cnt;
            }
        };
        put(ch.vec, vec_blocks, vec_capacity, nv);
        put(ch.mfma, mfma_blocks, mfma_capacity, nm);
        for (const PrefixBlock& b : ch.prefix) {
            if (prefix_blocks && np < prefix_capacity) {
                int32_t* w = prefix_blocks + 6 * (size_t)np;
                w[0] = (int32_t)c; w[1] = b.first; w[2] = b.q0; w[3] = b.len; w[4] = b.prefix_first; w[5] = b.prefix_len;
            }
            ++np;
        }
    }
    if (chunk_first_seq) chunk_first_seq[plan.chunks.size()] = n;
    for (size_t g = 0; g < plan.groups.size(); ++g)
        if (groups && (int32_t)g < group_capacity) {
            int32_t* w = groups + 4 * g;
            w[0] = plan.groups[g].chunk; w[1] = plan.groups[g].first_seq; w[2] = plan.groups[g].n_seq; w[3] = plan.groups[g].prefix;
        }
    *n_chunks = (int32_t)plan.chunks.size();
    *n_groups = (int32_t)plan.groups.size();
    *n_vec = nv;
    *n_mfma = nm;
    *n_prefix = np;
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_score_plan(const uint32_t* ids, const int32_t* offsets, const int32_t* firsts, int32_t n, int32_t head_dim,
                                                    int32_t min_shared, int32_t* chunk_first_seq, int32_t* chunk_rows, int32_t* n_chunks,
                                                    int32_t* groups, int32_t group_capacity, int32_t* n_groups, int32_t* vec_blocks,
                                                    int32_t vec_capacity, int32_t* n_vec, int32_t* mfma_blocks, int32_t mfma_capacity,
                                                    int32_t* n_mfma, int32_t* prefix_blocks, int32_t prefix_capacity, int32_t* n_prefix,
                                                    int32_t* gather, int32_t gather_capacity, int32_t* n_gather)
{
    if ((n > 0 && (!ids || !offsets || !firsts)) || !n_chunks || !n_groups || !n_vec || !n_mfma || !n_prefix || !n_gather)
        return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        if (n < 0 || group_capacity < 0 || vec_capacity < 0 || mfma_capacity < 0 || prefix_capacity < 0 || gather_capacity < 0)
            throw InvalidConfig("n and the capacities must not be negative");
        const ScorePlan plan = score_plan_host(ids, offsets, firsts, n, head_dim, min_shared);
        put_plan_tables(plan, n, chunk_first_seq, chunk_rows, n_chunks, groups, group_capacity, n_groups, vec_blocks, vec_capacity, n_vec,
                        mfma_blocks, mfma_capacity, n_mfma, prefix_blocks, prefix_capacity, n_prefix);
        int32_t ng = 0;
        for (size_t c = 0; c < plan.chunks.size(); ++c) {
            const ScoreChunk& ch = plan.chunks[c];
            for (size_t j = 0; j < ch.gather_src.size(); ++j) {
                if (gather && ng < gather_capacity) {
                    int32_t* w = gather + 4 * (size_t)ng;
                    w[0] = (int32_t)c; w[1] = ch.gather_src[j]; w[2] = ch.gather_tgt[j]; w[3] = ch.gather_slot[j];
                }
                ++ng;
            }
        }
        *n_gather = ng;
    });
}

// ---- answer logits ---------------------------------------------------------------------------------------------------------

static_assert(kAnswerMaxTargets == KJARNI_HIP_ANSWER_MAX_TARGETS, "the header's limit is the kernel's");

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_answer_logits(KjarniHipDecoder* d, const uint32_t* ids, const int32_t* offsets,
                                                               int32_t n_sequences, const uint32_t* targets, int32_t n_targets,
                                                               float* logits_out)
{
    if (!d || !targets || (n_sequences > 0 && (!ids || !offsets || !logits_out))) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->answer_logits_batch(ids, offsets, n_sequences, targets, n_targets, logits_out);  // checked before any GPU work
    });
}

KJARNI_EXPORT void kjarni_hip_decoder_answer_rows(const KjarniHipDecoder* d, uint64_t* computed, uint64_t* saved)
{
    if (computed) *computed = d ? d->model->answer_rows() : 0;
    if (saved) *saved = d ? d->model->answer_saved_rows() : 0;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_answer_plan(const uint32_t* ids, const int32_t* offsets, int32_t n, int32_t head_dim, int32_t min_shared,
                                                     int32_t* chunk_first_seq, int32_t* chunk_rows, int32_t* n_chunks, int32_t* groups,
                                                     int32_t group_capacity, int32_t* n_groups, int32_t* vec_blocks, int32_t vec_capacity,
                                                     int32_t* n_vec, int32_t* mfma_blocks, int32_t mfma_capacity, int32_t* n_mfma,
                                                     int32_t* prefix_blocks, int32_t prefix_capacity, int32_t* n_prefix, int32_t* gather,
                                                     int32_t gather_capacity, int32_t* n_gather)
{
    if ((n > 0 && (!ids || !offsets)) || !n_chunks || !n_groups || !n_vec || !n_mfma || !n_prefix || !n_gather) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        if (n < 0 || group_capacity < 0 || vec_capacity < 0 || mfma_capacity < 0 || prefix_capacity < 0 || gather_capacity < 0)
            throw InvalidConfig("n and the capacities must not be negative");
        const ScorePlan plan = answer_plan_host(ids, offsets, n, head_dim, min_shared);
        put_plan_tables(plan, n, chunk_first_seq, chunk_rows, n_chunks, groups, group_capacity, n_groups, vec_blocks, vec_capacity, n_vec,
                        mfma_blocks, mfma_capacity, n_mfma, prefix_blocks, prefix_capacity, n_prefix);
        int32_t ng = 0;
        for (size_t c = 0; c < plan.chunks.size(); ++c) {
            const ScoreChunk& ch = plan.chunks[c];
            for (size_t j = 0; j < ch.gather_src.size(); ++j) {  // (chunk, the chunk row of the sequence's last token, the sequence)
                if (gather && ng < gather_capacity) {
                    int32_t* w = gather + 3 * (size_t)ng;
                    w[0] = (int32_t)c; w[1] = ch.gather_src[j]; w[2] = ch.gather_slot[j];
                }
                ++ng;
            }
        }
        *n_gather = ng;
    });
}

// ---- embedding --------------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_embed(KjarniHipDecoder* d, const uint32_t* ids, const int32_t* offsets, int32_t n_sequences,
                                                       int32_t normalize, float* out)
{
    if (!d || (n_sequences > 0 && (!ids || !offsets || !out))) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->embed_batch(ids, offsets, n_sequences, normalize != 0, out);  // arguments checked before any GPU work
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_embed_plan(const int32_t* lengths, int32_t n, int32_t head_dim, int32_t* chunk_first_seq,
                                                    int32_t* n_chunks, int32_t* vec_blocks, int32_t vec_capacity, int32_t* n_vec,
                                                    int32_t* mfma_blocks, int32_t mfma_capacity, int32_t* n_mfma)
{
    if ((n > 0 && !lengths) || !n_chunks || !n_vec || !n_mfma) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        if (n < 0 || vec_capacity < 0 || mfma_capacity < 0) throw InvalidConfig("n and the capacities must not be negative");
        const std::vector<EmbedChunk> chunks = embed_plan_host(lengths, n, head_dim);
        int32_t nv = 0, nm = 0;
        for (size_t c = 0; c < chunks.size(); ++c) {
            if (chunk_first_seq) chunk_first_seq[c] = chunks[c].first_seq;
            auto put = [&](const std::vector<EmbedBlock>& src, int32_t* dst, int32_t cap, int32_t& cnt) {
                for (const EmbedBlock& b : src) {
                    if (dst && cnt < cap) {
                        int32_t* w = dst + 4 * (size_t)cnt;
                        w[0] = (int32_t)c; w[1] = b.first; w[2] = b.q0; w[3] = b.len;
                    }
                    ++cnt;
                }
            };
            put(chunks[c].vec, vec_blocks, vec_capacity, nv);
            put(chunks[c].mfma, mfma_blocks, mfma_capacity, nm);
        }
        if (chunk_first_seq) chunk_first_seq[chunks.size()] = n;
        *n_chunks = (int32_t)chunks.size();
        *n_vec = nv;
        *n_mfma = nm;
    });
}

// ---- prefix reuse -----------------------------------------------------------------------------------------------------------

KJARNI_EXPORT void kjarni_hip_decoder_set_prefix_reuse(KjarniHipDecoder* d, int32_t on)
{
    if (!d) return;
    std::lock_guard<std::mutex> lock(d->mu);
    d->model->set_prefix_reuse(on != 0);
}

// ---- FP8 checkpoints on the matrix cores (LlmModel::set_fp8_matrix_cores) ------------------------------------------------------

KJARNI_EXPORT void kjarni_hip_decoder_set_fp8_matrix_cores(KjarniHipDecoder* d, int32_t on)
{
    if (!d) return;
    std::lock_guard<std::mutex> lock(d->mu);
    (void)guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { d->model->set_fp8_matrix_cores(on != 0); });
}

KJARNI_EXPORT int32_t kjarni_hip_decoder_fp8_matrix_cores(const KjarniHipDecoder* d) { return d && d->model->fp8_matrix_cores() ? 1 : 0; }

KJARNI_EXPORT void kjarni_hip_decoder_prefix_stats(const KjarniHipDecoder* d, uint64_t* reused, uint64_t* computed)
{
    if (reused) *reused = d ? d->model->prefix_reused_tokens() : 0;
    if (computed) *computed = d ? d->model->prefix_computed_tokens() : 0;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_resident(const KjarniHipDecoder* d, uint32_t* out, size_t capacity, size_t* n)
{
    if (!d || !n || (capacity && !out)) return KJARNI_ERROR_NULL_POINTER;
    std::lock_guard<std::mutex> lock(d->mu);
    const std::vector<uint32_t>& r = d->model->resident();
    *n = r.size();
    if (capacity) std::memcpy(out, r.data(), std::min(capacity, r.size()) * sizeof(uint32_t));
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_last_logits(const KjarniHipDecoder* d, float* logits_out)
{
    if (!d || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->logits_to_host(logits_out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_prefix_keep(const uint32_t* resident, size_t n, const uint32_t* prompt, size_t m, size_t limit,
                                                     size_t* keep)
{
    if (!keep || (n && !resident) || (m && !prompt)) return KJARNI_ERROR_NULL_POINTER;
    *keep = prefix_keep_host(resident, n, prompt, m, limit);
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_generation_replay(size_t n_prompt, size_t capacity, size_t max_new_tokens, size_t max_len,
                                                       const uint32_t* stop_ids, size_t n_stop, const uint32_t* default_stop_ids,
                                                       size_t n_default_stop, const uint32_t* stream, size_t n_stream, int64_t cancel_after,
                                                       int32_t feed_last, size_t* n_emitted, size_t* n_asked, size_t* n_fed)
{
    if (!n_emitted || !n_asked || (n_stop && !stop_ids) || (n_default_stop && !default_stop_ids) || (n_stream && !stream))
        return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] {
        GenerateOptions opt;
        opt.max_new_tokens = max_new_tokens;
        opt.max_len = max_len;
        opt.stop_ids.assign(stop_ids, stop_ids + n_stop);
        std::vector<uint32_t> out;
        GenerationRun run(std::vector<uint32_t>(n_prompt, 0u), opt, capacity, std::vector<uint32_t>(default_stop_ids, default_stop_ids + n_default_stop),
                          out);
        const std::function<bool(uint32_t)> cb = [&](uint32_t) { return cancel_after < 0 || (int64_t)out.size() != cancel_after; };
        size_t asked = 0, fed = 0;
        while (run.wants_token() && asked < n_stream)
            if (run.accept(stream[asked++], cb) && run.feeds_accepted(feed_last ? LastToken::Fed : LastToken::NotFed)) ++fed;
        *n_emitted = out.size();
        *n_asked = asked;
        if (n_fed) *n_fed = fed;
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_lane_prefill_shared(KjarniHipDecoder* d, int32_t lane, int32_t shared, const uint32_t* ids,
                                                                     int32_t n)
{
    if (!d || !ids) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        std::lock_guard<std::mutex> lock(d->mu);
        d->model->lane_prefill_shared(LlmModel::Bank::Lanes, lane, shared, ids, n);  // ranges checked before any GPU work
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_config_json(const KjarniHipDecoder* d, char** out)
{
    if (!d || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_UNKNOWN, [&] { *out = dup_cstr(d->model->config_json()); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_decoder_weight_bytes_by_type(const KjarniHipDecoder* d, uint64_t* out, size_t n)
{
    if (!d || (n && !out)) return KJARNI_ERROR_NULL_POINTER;
    for (size_t t = 0; t < n; ++t) out[t] = d->model->weight_bytes_of_type((int)t);
    return KJARNI_OK;
}

static_assert(KJARNI_HIP_WEIGHT_TYPE_F8_E4M3 == kFp8WeightType && KJARNI_HIP_WEIGHT_TYPE_F8_E4M3 < 32, "the FP8 entry of the per-type byte counts");

KJARNI_EXPORT KjarniErrorCode kjarni_fp8_tensor_f32(const char* model_dir, const char* hf_name, float* out, size_t capacity, size_t* n_out,
                                                    int64_t* shape_out, int32_t* ndim_out)
{
    if (!model_dir || !hf_name || !n_out || (capacity && !out)) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        const std::string dir = model_dir;
        SafeTensors st;
        st.open_dir(dir);
        std::string config;
        {
            std::ifstream f(dir + "/config.json", std::ios::binary);
            if (f) config.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        }
        const Fp8Checkpoint f8(st, config);
        if (!st.contains(hf_name)) throw std::runtime_error(std::string("tensor not found: ") + hf_name);
        std::vector<float> v;
        const std::vector<int64_t> shape = f8.read_f32(hf_name, v);
        *n_out = v.size();
        if (ndim_out) *ndim_out = (int32_t)shape.size();
        if (shape_out) {
            shape_out[0] = shape[0];
            shape_out[1] = shape[1];
        }
        if (capacity) std::memcpy(out, v.data(), std::min(capacity, v.size()) * sizeof(float));
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_gguf_config_json(const char* path, char** out)
{
    if (!path || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        const std::string f = resolve_gguf(path);
        if (f.empty()) throw ModelNotFound(std::string("no GGUF file at ") + path);
        GgufFile g;
        g.open(f);
        *out = dup_cstr(g.config_json());
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_gguf_tensor_f32(const char* path, const char* hf_name, float* out, size_t capacity, size_t* n_out,
                                                     int64_t* shape_out, int32_t* ndim_out)
{
    if (!path || !hf_name || !n_out || (capacity && !out)) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        const std::string f = resolve_gguf(path);
        if (f.empty()) throw ModelNotFound(std::string("no GGUF file at ") + path);
        GgufFile g;
        g.open(f);
        std::vector<float> v;
        const std::vector<int64_t> shape = g.read_f32(hf_name, v);
        *n_out = v.size();
        if (ndim_out) *ndim_out = (int32_t)shape.size();
        if (shape_out) {
            shape_out[0] = shape.size() == 2 ? shape[0] : 1;
            shape_out[1] = shape.back();
        }
        if (capacity) std::memcpy(out, v.data(), std::min(capacity, v.size()) * sizeof(float));
    });
}
