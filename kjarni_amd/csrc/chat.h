// Chat: prompt templating, generation-config resolution and the text side of the decoder generation loop.
//
//   templates            crates/kjarni-transformers/src/chat/{llama3.rs:38-96, chatml.rs:15-48, mistral.rs:16-80}
//   Conversation/History crates/kjarni-transformers/src/chat/templates.rs:51-131, crates/kjarni/src/chat/types.rs:197-238
//   Chat                 crates/kjarni/src/chat/model.rs:30-352 (builder defaults: chat/builder.rs, modes: chat/types.rs:122-146)
//   config resolution    crates/kjarni/src/generation/resolution.rs:8-85
//   model defaults       crates/kjarni-models/src/models/{llama/model.rs:373-396, qwen/model.rs:261-282},
//                        crates/kjarni-transformers/src/common/mod.rs:297-349 (generation_config.json)
//   encode / stop ids    crates/kjarni-transformers/src/decoder/generator.rs:141-163, models/base.rs:261-271
//   token text, cleanup  decoder/generator.rs:343-360, crates/kjarni/src/chat/model.rs:283-303
//   Generator            crates/kjarni/src/generator/{model.rs:40-250, validation.rs:8-51} (raw completion, no template)
#pragma once
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "bpe.h"
#include "constraint_kernels.h"
#include "grammar_kernels.h"
#include "llm.h"
#include "registry.h"
#include "sampling.h"

namespace kjarni {

enum class ChatTemplateKind { Llama3 = 0, ChatML = 1, Mistral = 2 };
enum class ChatRole { System = 0, User = 1, Assistant = 2 };

struct ChatMessage {
    ChatRole role;
    std::string content;
};

std::string apply_chat_template(ChatTemplateKind kind, const std::vector<ChatMessage>& conversation);
std::vector<std::string> chat_stop_sequences(ChatTemplateKind kind);
const char* chat_default_system_prompt(ChatTemplateKind kind);  // nullptr when the template has none

template <class T>
struct Opt {
    bool has = false;
    T value{};
    Opt() = default;
    Opt(const T& v) : has(true), value(v) {}
    Opt or_else(const Opt& other) const { return has ? *this : other; }
};

struct GenerationOverrides {
    Opt<float> temperature, top_p, min_p, repetition_penalty, length_penalty;
    Opt<size_t> top_k, no_repeat_ngram_size, max_new_tokens, num_beams;
    Opt<bool> do_sample;
};

enum class Strategy { Greedy = 0, Sample = 1, BeamSearch = 2 };

struct GenerationConfig {
    Opt<size_t> max_new_tokens;
    size_t max_length = 0;
    float repetition_penalty = 1.0f;
    size_t no_repeat_ngram_size = 0;
    bool add_bos_token = true;
    Strategy strategy = Strategy::Greedy;
    // SamplingParams (temperature 0.7, top_k 50, top_p 0.9 are SamplingParams::default())
    float temperature = 0.7f;
    Opt<size_t> top_k;
    Opt<float> top_p, min_p;
    size_t num_beams = 4;  // BeamSearchParams::default()
    float length_penalty = 1.0f;
};

GenerationConfig resolve_generation_config(GenerationConfig model_defaults, const GenerationOverrides& user,
                                           const GenerationOverrides& runtime);
// get_default_generation_config: generation_config.json when it parses, the per-architecture fallback otherwise.
GenerationConfig model_default_generation_config(const std::string& model_type, size_t max_position_embeddings,
                                                 const std::string* generation_config_json);

// The tokens a handle's last request emitted and their log-probability records (Chat / Generator::last_logprobs).
struct GeneratedLogprobs {
    std::vector<uint32_t> tokens;
    TokenLogprobs records;
};

class Chat {
public:
    // model_name: registry name (decides architecture, template and the on-disk directory); model_dir overrides the
    // directory.  mode: 0 default, 1 creative, 2 reasoning.
    static std::unique_ptr<Chat> create(const std::string& model_name, const std::string& model_dir, const std::string& cache_dir,
                                        const std::string* system_prompt, int mode, bool quiet);

    const std::string& model_name() const { return model_name_; }
    size_t context_size() const { return (size_t)model_->config().max_pos; }
    const std::string* system_prompt() const { return has_system_ ? &system_prompt_ : nullptr; }
    ChatTemplateKind template_kind() const { return template_; }
    const BpeTokenizer& tokenizer() const { return tokenizer_; }
    LlmModel& model() { return *model_; }

    std::string format_prompt(const std::vector<ChatMessage>& conversation) const { return apply_chat_template(template_, conversation); }
    std::vector<ChatMessage> create_conversation() const;  // Chat::create_conversation
    std::vector<ChatMessage> history_to_conversation(const std::vector<ChatMessage>& history) const;
    GenerationConfig resolve(const GenerationOverrides& runtime) const;
    std::vector<uint32_t> encode(const std::string& prompt, const GenerationConfig& config) const;  // DecoderGenerator::encode

    // Generator::generate_with_config + Chat::generate: concatenated token texts, trimmed, stop sequences stripped.
    std::string generate(const std::string& prompt, const GenerationOverrides& runtime);
    // generate_stream: on_text per generated token (return false to stop); returns the concatenation of what was emitted.
    std::string generate_stream(const std::string& prompt, const GenerationOverrides& runtime,
                                const std::function<bool(const std::string&)>& on_text);
    void reseed(uint64_t seed) { rng_.reseed(seed); }
    // Prompt-lookup decoding for sampled requests (LlmModel::generate_lookup_sampled, the default draft length): off by default;
    // a request with an n-gram ban and every greedy request keep the plain loop.
    void set_prompt_lookup_sampling(bool on) { lookup_sampling_ = on; }
    // A draft model for send (LlmModel::generate_draft): `path` (a model directory or a .gguf) is loaded on the model's device
    // with its weights as stored and the model's context, and owned by the handle; an empty path or draft_tokens == 0 frees it.
    // While set it takes precedence over prompt lookup.  InvalidConfig for draft_tokens outside 0..7 or another vocabulary.
    void set_draft_model(const std::string& path, int draft_tokens);
    // Constrained decoding (LlmModel::generate with a constraint): every later request emits only what `pattern` (constraint.h's
    // syntax) matches in full; an empty pattern restores the plain behaviour.  The token table is built from the handle's
    // tokenizer (BpeTokenizer::token_bytes over the model's vocabulary) once per pattern and the compiled constraint is kept until
    // the pattern changes.  While set, requests take the plain loop even when prompt lookup or a draft model is switched on.
    // InvalidConfig for a pattern the compiler refuses.  Nested or recursive formats (JSON schemas) are out of scope.
    void set_constraint(const std::string& pattern);
    ConstraintOutcome constraint_outcome() const { return constraint_outcome_; }  // of the last constrained request
    // The same with a grammar (grammar.h: rules (name, pattern), rule 0 the start rule) in the pattern's place; no rule removes it.
    // A handle holds a pattern or a grammar: setting one clears the other.  constraint_outcome() reports either kind of request.
    void set_grammar(const std::vector<std::pair<std::string, std::string>>& rules);
    // Log-probabilities of the generated tokens (GenerateOptions::logprobs): -1 = off (the default), 0..KJARNI_SCORE_TOPK_MAX = every
    // later request records, per emitted token, its log-probability under the raw distribution and that many alternatives.  While
    // set, requests take the plain loop even when prompt lookup or a draft model is switched on (as under a constraint).
    // InvalidConfig for a value outside -1..KJARNI_SCORE_TOPK_MAX or above the vocabulary.
    void set_logprobs(int top_k);
    int logprobs() const { return logprobs_; }
    // The tokens of the last request and their records (empty before any request, and after one that ran with logprobs off).
    GeneratedLogprobs last_logprobs() const;

private:
    Chat() = default;
    std::string run(const std::string& prompt, const GenerationOverrides& runtime, const std::function<bool(const std::string&)>& on_text);

    std::string model_name_;
    std::unique_ptr<LlmModel> model_;
    BpeTokenizer tokenizer_;
    ChatTemplateKind template_ = ChatTemplateKind::Llama3;
    bool has_system_ = false;
    std::string system_prompt_;
    int mode_ = 0;
    GenerationConfig generation_config_;   // Generator::generation_config (model defaults + mode)
    GenerationOverrides mode_overrides_;   // Generator::user_overrides
    std::vector<uint32_t> stop_ids_;
    UniformRng rng_;
    bool lookup_sampling_ = false;
    std::unique_ptr<LlmModel> drafter_;
    int draft_tokens_ = 0;
    std::string constraint_pattern_;
    std::unique_ptr<DeviceConstraint> constraint_;
    std::unique_ptr<DeviceGrammar> grammar_;
    ConstraintOutcome constraint_outcome_;
    int logprobs_ = -1;
    GeneratedLogprobs last_logprobs_;
    mutable std::mutex mutex_;  // one generation at a time per handle (the KV cache is the handle's)
};

// Raw text completion (the reference's Generator): validation, model defaults (GenerationConfig::default() for GPT-2) and the
// same token loop as Chat, with no template, no trimming and no stop-sequence stripping.
class Generator {
public:
    // model_name: registry name (Llama, Qwen2, Mistral, GPT); model_dir overrides the directory.  Checks run in Chat::create's
    // order: the name, the files on disk, Phi-3, then the load (the first GPU call).
    static std::unique_ptr<Generator> create(const std::string& model_name, const std::string& model_dir, const std::string& cache_dir,
                                             bool quiet);

    const std::string& model_name() const { return model_name_; }
    size_t context_size() const { return (size_t)model_->config().max_pos; }
    size_t vocab_size() const { return (size_t)model_->config().vocab; }
    LlmModel& model() { return *model_; }
    GenerationConfig resolve(const GenerationOverrides& runtime) const;
    std::vector<uint32_t> encode(const std::string& prompt, const GenerationConfig& config) const;  // DecoderGenerator::encode

    // Generator::generate_with_config: the concatenated single-token decodes of the generated tokens, as they are.
    std::string generate(const std::string& prompt, const GenerationOverrides& runtime) { return run(prompt, runtime, nullptr); }
    std::string generate_stream(const std::string& prompt, const GenerationOverrides& runtime,
                                const std::function<bool(const std::string&)>& on_text)
    {
        return run(prompt, runtime, on_text);
    }
    void reseed(uint64_t seed) { rng_.reseed(seed); }
    // generate() for every prompt, up to `lanes` (1..8, 0 = 8) of them decoded in lock step; texts in prompt order.
    std::vector<std::string> generate_batch(const std::vector<std::string>& prompts, const GenerationOverrides& runtime, int lanes);
    int batch_lanes() const { return batch_lanes_; }
    void set_batch_lanes(int lanes) { batch_lanes_ = lanes; }  // what kjarni_generator_generate_batch runs with (0 = 8)
    // 1..64: generate_batch runs LlmModel::generate_wide with that width instead of generate_lanes; 0 (the default) = off
    int wide_lanes() const { return wide_lanes_; }
    void set_wide_lanes(int lanes) { wide_lanes_ = lanes; }
    // Prompt-lookup decoding for generate / stream (0 = off, the default; 1..7 drafted tokens per step): used when the resolved
    // config is greedy without a repetition penalty or an n-gram ban (LlmModel::generate_lookup); generate_batch is untouched.
    void set_prompt_lookup(int draft_tokens) { prompt_lookup_ = draft_tokens; }
    int prompt_lookup() const { return prompt_lookup_; }
    // The same for sampled configs, with or without a repetition penalty (LlmModel::generate_lookup_sampled): off by default;
    // taken when it is on, prompt lookup is set and the resolved config has no n-gram ban.
    void set_prompt_lookup_sampling(bool on) { lookup_sampling_ = on; }
    // A draft model for generate / stream (Chat::set_draft_model's contract); generate_batch is untouched.
    void set_draft_model(const std::string& path, int draft_tokens);
    // Constrained decoding for generate / stream (Chat::set_constraint's contract).  generate_batch passes the handle's pattern or
    // grammar to every prompt of the batch (LlmModel::generate_lanes / generate_wide take one per request) and keeps one outcome
    // per prompt.
    void set_constraint(const std::string& pattern);
    ConstraintOutcome constraint_outcome() const { return constraint_outcome_; }
    // Prompt `prompt_index` of the last generate_batch call: *kind 0 none, 1 pattern, 2 grammar, and its outcome (zeros with kind 0
    // before a call, after an unconstrained one and for an index the call did not have).
    ConstraintOutcome batch_constraint_outcome(size_t prompt_index, int* kind) const;
    // Test hook: the seed of the generator prompt `prompt_index` of the last generate_batch call drew from (0: no such prompt).
    // reseed() with it and generate() of that prompt alone take the same draws.
    uint64_t batch_seed(size_t prompt_index) const;
    void set_grammar(const std::vector<std::pair<std::string, std::string>>& rules);  // (Chat::set_grammar's contract)
    // Log-probabilities of the generated tokens (GenerateOptions::logprobs): -1 = off (the default), 0..KJARNI_SCORE_TOPK_MAX = every
    // later request records, per emitted token, its log-probability under the raw distribution and that many alternatives.  While
    // set, requests take the plain loop even when prompt lookup or a draft model is switched on (as under a constraint).
    // InvalidConfig for a value outside -1..KJARNI_SCORE_TOPK_MAX or above the vocabulary.
    void set_logprobs(int top_k);
    int logprobs() const { return logprobs_; }
    // The tokens and records of prompt `prompt_index` of the last generate / stream (index 0) / generate_batch call; empty before
    // any call, after a call that ran with logprobs off, and for an index the call did not have.
    GeneratedLogprobs last_logprobs(size_t prompt_index) const;
    // The log-likelihood of `continuation` after `context` (LlmModel::score).  Tokens as lm-eval-harness takes them, with
    // encode() under the model's default config: whole = encode(context + continuation), first = len(encode(context)), scored
    // whole[first:].  InvalidConfig, nothing truncated: no context token (empty context, model without BOS), a continuation
    // that adds no token, more tokens than the model's context.
    struct Score {
        double sum_logprob = 0.0;  // the f32 log-probabilities summed in order, in double
        size_t n_tokens = 0;
        bool is_greedy = false;    // every scored token is its position's arg-max
    };
    Score score(const std::string& context, const std::string& continuation);
    // score() token by token, with the top_k most likely tokens of every scored position (LlmModel::score_topk): the same
    // tokens and the same errors, plus InvalidConfig for top_k outside [1, KJARNI_SCORE_TOPK_MAX] or above the vocabulary.
    struct TokenScores {
        std::vector<uint32_t> tokens;       // whole[first:]
        std::vector<float> logprobs;        // [n_tokens]
        std::vector<uint32_t> top_tokens;   // [n_tokens, top_k]
        std::vector<float> top_logprobs;    // [n_tokens, top_k]
        size_t top_k = 0;
    };
    TokenScores score_tokens(const std::string& context, const std::string& continuation, size_t top_k);
    // score() for every (context, continuation) pair.  All pairs are encoded and checked by score()'s rules first: a failure is
    // the call's InvalidConfig with the pair's index in front of the reason, and nothing is computed.  The pairs the packed path
    // takes run through LlmModel::score_batch in the caller's order (neighbouring pairs that repeat a context share its rows);
    // the others -- pairs longer than LlmModel::embed_max_tokens(), or every pair on a checkpoint score_batch refuses -- through
    // LlmModel::score one by one.
    std::vector<Score> score_batch(const std::vector<std::pair<std::string, std::string>>& pairs);

private:
    Generator() = default;
    // score()'s token rule and checks: whole = encode(context + continuation), returns first = len(encode(context))
    size_t encode_scored(const std::string& context, const std::string& continuation, std::vector<uint32_t>& whole) const;
    std::string run(const std::string& prompt, const GenerationOverrides& runtime, const std::function<bool(const std::string&)>& on_text);

    std::string model_name_;
    std::unique_ptr<LlmModel> model_;
    BpeTokenizer tokenizer_;
    GenerationConfig generation_config_;  // the model's defaults (no builder overrides through the C ABI)
    std::vector<uint32_t> stop_ids_;
    UniformRng rng_;
    mutable std::mutex mutex_;
    int batch_lanes_ = 0, wide_lanes_ = 0;
    int prompt_lookup_ = 0;
    bool lookup_sampling_ = false;
    std::unique_ptr<LlmModel> drafter_;
    int draft_tokens_ = 0;
    std::string constraint_pattern_;
    std::unique_ptr<DeviceConstraint> constraint_;
    std::unique_ptr<DeviceGrammar> grammar_;
    ConstraintOutcome constraint_outcome_;
    std::vector<ConstraintOutcome> batch_outcomes_;  // of the last generate_batch call under batch_kind_ (empty: unconstrained)
    int batch_kind_ = 0;
    std::vector<uint64_t> batch_seeds_;
    int logprobs_ = -1;
    std::vector<GeneratedLogprobs> last_logprobs_;
};

// str::trim (Unicode White_Space at both ends).
std::string trim_unicode(const std::string& s);

}  // namespace kjarni
