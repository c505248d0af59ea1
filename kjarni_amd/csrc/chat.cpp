// Chat host logic (see chat.h for the reference files each part follows).
#include "chat.h"

#include <sys/stat.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "ffi_common.h"
#include "json.h"
#include "unicode.h"

namespace kjarni {

// ---- templates ------------------------------------------------------------------------------------

namespace {
const char* role_name(ChatRole r) { return r == ChatRole::System ? "system" : (r == ChatRole::User ? "user" : "assistant"); }
}  // namespace

std::string apply_chat_template(ChatTemplateKind kind, const std::vector<ChatMessage>& conv)
{
    std::string p;
    switch (kind) {
    case ChatTemplateKind::Llama3:  // llama3.rs:57-75, for_generation(): BOS and the assistant header are added
        p += "<|begin_of_text|>";
        for (const ChatMessage& m : conv) {
            p += "<|start_header_id|>";
            p += role_name(m.role);
            p += "<|end_header_id|>\n\n";
            p += m.content;
            p += "<|eot_id|>";
        }
        p += "<|start_header_id|>assistant<|end_header_id|>\n\n";
        break;
    case ChatTemplateKind::ChatML:  // chatml.rs:15-34
        for (const ChatMessage& m : conv) {
            p += "<|im_start|>";
            p += role_name(m.role);
            p += "\n";
            p += m.content;
            p += "<|im_end|>\n";
        }
        p += "<|im_start|>assistant\n";
        break;
    case ChatTemplateKind::Mistral: {  // mistral.rs:16-75
        if (conv.empty()) return p;
        p += "<s>";
        size_t i = 0;
        const std::string* system = nullptr;
        if (conv[0].role == ChatRole::System) {
            system = &conv[0].content;
            i = 1;
        }
        bool first_user = true;
        for (; i < conv.size(); ++i) {
            const ChatMessage& m = conv[i];
            if (m.role == ChatRole::User) {
                p += "[INST] ";
                if (first_user) {
                    if (system) {
                        p += *system;
                        p += "\n\n";
                    }
                    first_user = false;
                }
                p += m.content;
                p += " [/INST]";
            } else if (m.role == ChatRole::Assistant) {
                p += ' ';
                p += m.content;
                p += "</s>";
            }
        }
        break;
    }
    }
    return p;
}

std::vector<std::string> chat_stop_sequences(ChatTemplateKind kind)
{
    switch (kind) {
    case ChatTemplateKind::Llama3: return {"<|eot_id|>", "<|end_of_text|>"};
    case ChatTemplateKind::ChatML: return {"<|im_end|>", "<|endoftext|>"};
    case ChatTemplateKind::Mistral: return {"</s>"};
    }
    return {};
}

const char* chat_default_system_prompt(ChatTemplateKind kind)
{
    switch (kind) {
    case ChatTemplateKind::Llama3: return "You are a helpful, harmless, and honest assistant.";
    case ChatTemplateKind::ChatML: return "You are a helpful assistant.";
    case ChatTemplateKind::Mistral: return nullptr;
    }
    return nullptr;
}

std::string trim_unicode(const std::string& s)
{
    std::vector<uint32_t> cps;
    if (!unicode::decode_utf8(s.data(), s.size(), cps)) return s;
    size_t a = 0, b = cps.size();
    while (a < b && unicode::is_whitespace(cps[a])) ++a;
    while (b > a && unicode::is_whitespace(cps[b - 1])) --b;
    return unicode::encode_utf8(std::vector<uint32_t>(cps.begin() + (ptrdiff_t)a, cps.begin() + (ptrdiff_t)b));
}

// ---- generation config ----------------------------------------------------------------------------

GenerationConfig resolve_generation_config(GenerationConfig config, const GenerationOverrides& user, const GenerationOverrides& runtime)
{
    const Opt<size_t> beams = runtime.num_beams.or_else(user.num_beams);
    const bool force_beams = beams.has && beams.value > 1;
    const Opt<bool> sample = runtime.do_sample.or_else(user.do_sample);
    const bool force_greedy = sample.has && !sample.value;
    const bool force_sampling = sample.has && sample.value;

    if (force_beams) {
        if (config.strategy != Strategy::BeamSearch) {  // BeamSearchParams::default()
            config.num_beams = 4;
            config.length_penalty = 1.0f;
        }
        config.strategy = Strategy::BeamSearch;
    } else if (force_greedy) {
        config.strategy = Strategy::Greedy;
    } else if (force_sampling) {
        if (config.strategy != Strategy::Sample) {  // SamplingParams::default()
            config.temperature = 0.7f;
            config.top_k = Opt<size_t>(50);
            config.top_p = Opt<float>(0.9f);
            config.min_p = Opt<float>(0.1f);
        }
        config.strategy = Strategy::Sample;
    }
    if (const auto v = runtime.max_new_tokens.or_else(user.max_new_tokens); v.has) config.max_new_tokens = v;
    if (const auto v = runtime.repetition_penalty.or_else(user.repetition_penalty); v.has) config.repetition_penalty = v.value;
    if (const auto v = runtime.no_repeat_ngram_size.or_else(user.no_repeat_ngram_size); v.has) config.no_repeat_ngram_size = v.value;
    if (config.strategy == Strategy::Sample) {
        if (const auto v = runtime.temperature.or_else(user.temperature); v.has) config.temperature = v.value;
        if (const auto v = runtime.top_k.or_else(user.top_k); v.has) config.top_k = v;
        if (const auto v = runtime.top_p.or_else(user.top_p); v.has) config.top_p = v;
        if (const auto v = runtime.min_p.or_else(user.min_p); v.has) config.min_p = v;
    } else if (config.strategy == Strategy::BeamSearch) {
        if (beams.has) config.num_beams = beams.value;
        if (const auto v = runtime.length_penalty.or_else(user.length_penalty); v.has) config.length_penalty = v.value;
    }
    return config;
}

GenerationConfig model_default_generation_config(const std::string& model_type, size_t max_pos, const std::string* hf_json)
{
    GenerationConfig c;
    if (model_type == "gpt2") {
        // Gpt2Model keeps the trait's default (decoder/traits.rs:283-285): GenerationConfig::default()
        // (common/mod.rs:78-96), whatever generation_config.json says
        c.max_new_tokens = Opt<size_t>(50);
        c.max_length = 100;
        c.repetition_penalty = 1.0f;
        c.no_repeat_ngram_size = 0;
        c.add_bos_token = true;
        c.strategy = Strategy::Sample;
        c.temperature = 0.7f;
        c.top_k = Opt<size_t>(50);
        c.top_p = Opt<float>(0.9f);
        c.min_p = Opt<float>(0.1f);
        return c;
    }
    if (hf_json && model_type != "mistral") {  // HFGenerationDefaults (a file that does not deserialize is ignored); Mistral never reads it
        try {
            const Json j = Json::parse(*hf_json);
            if (!j.is_object()) throw std::runtime_error("not an object");
            auto typed = [&](const char* k, Json::Type t) {  // serde: a present field of the wrong type fails the whole file
                const Json* v = j.find(k);
                if (v && !v->is_null() && v->type != t) throw std::runtime_error("type");
                return v && !v->is_null() ? v : nullptr;
            };
            const Json* do_sample = typed("do_sample", Json::Bool);
            const Json* temperature = typed("temperature", Json::Number);
            const Json* top_p = typed("top_p", Json::Number);
            const Json* top_k = typed("top_k", Json::Number);
            const Json* max_new = typed("max_new_tokens", Json::Number);
            const Json* max_len = typed("max_length", Json::Number);
            const Json* rep = typed("repetition_penalty", Json::Number);
            typed("decoder_start_token_id", Json::Number);
            if (j.find("do_sample") && j.find("do_sample")->is_null()) throw std::runtime_error("do_sample: null");
            if (j.find("temperature") && j.find("temperature")->is_null()) throw std::runtime_error("temperature: null");
            if (do_sample && do_sample->as_bool()) {
                c.strategy = Strategy::Sample;
                c.temperature = temperature ? (float)temperature->as_double() : 1.0f;
                c.top_k = top_k ? Opt<size_t>((size_t)top_k->as_int()) : Opt<size_t>();
                c.top_p = top_p ? Opt<float>((float)top_p->as_double()) : Opt<float>();
                c.min_p = Opt<float>();
            } else {
                c.strategy = Strategy::Greedy;
            }
            c.max_new_tokens = max_new ? Opt<size_t>((size_t)max_new->as_int()) : Opt<size_t>();
            c.max_length = max_len ? (size_t)max_len->as_int() : max_pos;
            c.repetition_penalty = rep ? (float)rep->as_double() : 1.0f;
            c.no_repeat_ngram_size = 0;
            c.add_bos_token = true;
            return c;
        } catch (const std::exception&) {
        }
    }
    c.max_length = max_pos;
    c.no_repeat_ngram_size = 0;
    c.strategy = Strategy::Sample;
    if (model_type == "mistral") {  // mistral/model.rs:236-252
        c.max_new_tokens = Opt<size_t>(512);
        c.repetition_penalty = 1.15f;
        c.add_bos_token = true;
        c.temperature = 0.7f;
        c.top_k = Opt<size_t>(40);
        c.top_p = Opt<float>(0.9f);
        c.min_p = Opt<float>(0.05f);
    } else if (model_type == "qwen2" || model_type == "qwen3" || model_type == "qwen3_moe") {  // qwen/model.rs:267-281 (Qwen3: the Qwen2 block)
        c.max_new_tokens = Opt<size_t>(512);
        c.repetition_penalty = 1.1f;
        c.add_bos_token = false;
        c.temperature = 0.7f;
        c.top_k = Opt<size_t>(40);
        c.top_p = Opt<float>(0.8f);
        c.min_p = Opt<float>(0.05f);
    } else {  // llama/model.rs:381-395
        c.max_new_tokens = Opt<size_t>(256);
        c.repetition_penalty = 1.0f;
        c.add_bos_token = true;
        c.temperature = 0.6f;
        c.top_k = Opt<size_t>();
        c.top_p = Opt<float>(0.9f);
        c.min_p = Opt<float>(0.05f);
    }
    return c;
}

// ---- Chat -----------------------------------------------------------------------------------------

namespace {

struct ChatModelInfo {
    const char* cli_name;
    const char* arch;     // ModelArchitecture::display_name
    const char* family;   // llama | qwen2 | qwen3 | mistral | phi3 | gpt | encoder | whisper | seq2seq
    const char* task;     // format!("{:?}", task).to_lowercase()
};
// registry.rs ModelType::info(): architecture and task of every registry entry.
const ChatModelInfo kChatModels[] = {
    {"minilm-l6-v2", "BERT", "encoder", "embedding"},
    {"minilm-l6-v2-cross-encoder", "BERT", "encoder", "reranking"},
    {"mpnet-base-v2", "Mpnet", "encoder", "embedding"},
    {"distilbert-base", "BERT", "encoder", "embedding"},
    {"nomic-embed-text", "Nomic-BERT", "encoder", "embedding"},
    {"bge-m3", "BERT", "encoder", "embedding"},
    {"distilbert-sentiment", "BERT", "encoder", "sentimentanalysis"},
    {"roberta-sentiment", "BERT", "encoder", "sentimentanalysis"},
    {"bert-sentiment-multilingual", "BERT", "encoder", "sentimentanalysis"},
    {"roberta-emotions", "BERT", "encoder", "classification"},
    {"distilroberta-emotion", "BERT", "encoder", "classification"},
    {"toxic-bert", "BERT", "encoder", "classification"},
    {"qwen2.5-0.5b-instruct", "Qwen2 (Biased)", "qwen2", "chat"},
    {"qwen2.5-1.5b", "Qwen2 (Biased)", "qwen2", "chat"},
    {"qwen3-0.6b", "Qwen3 (QK-Norm)", "qwen3", "chat"},
    {"qwen3-1.7b", "Qwen3 (QK-Norm)", "qwen3", "chat"},
    {"qwen3-4b", "Qwen3 (QK-Norm)", "qwen3", "chat"},
    {"qwen3-8b", "Qwen3 (QK-Norm)", "qwen3", "chat"},
    {"qwen3-30b-a3b", "Qwen3-MoE (128 experts, 8 active)", "qwen3", "chat"},
    {"qwen3-30b-a3b-instruct-2507", "Qwen3-MoE (128 experts, 8 active)", "qwen3", "chat"},
    {"llama3.2-1b-instruct", "Llama (Standard)", "llama", "chat"},
    {"llama3.2-3b-instruct", "Llama (Standard)", "llama", "chat"},
    {"phi3.5-mini", "Phi-3 (LongRoPE)", "phi3", "reasoning"},
    {"mistral-7b", "Mistral (SWA)", "mistral", "chat"},
    {"llama3.1-8b-instruct", "Llama (Standard)", "llama", "chat"},
    {"deepseek-r1-8b", "Llama (Standard)", "llama", "reasoning"},
    {"flan-t5-base", "T5", "seq2seq", "seq2seq"},
    {"flan-t5-large", "T5", "seq2seq", "seq2seq"},
    {"bart-large-cnn", "BART", "seq2seq", "seq2seq"},
    {"distilbart-cnn", "BART", "seq2seq", "seq2seq"},
    {"whisper-small", "Whisper (ASR)", "whisper", "speechtotext"},
    {"whisper-large-v3", "Whisper (ASR)", "whisper", "speechtotext"},
    {"distilgpt2", "GPT", "gpt", "generation"},
    {"gpt2", "GPT", "gpt", "generation"},
};


bool read_file(const std::string& p, std::string& out)
{
    std::ifstream f(p, std::ios::binary);
    if (!f) return false;
    std::ostringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
}

const ChatModelInfo* model_info(const std::string& model_name, const RegistryEntry*& entry)
{
    std::string err;
    entry = resolve_model(model_name, err);
    if (!entry) throw ModelNotFound(err);  // ChatError::UnknownModel / GeneratorError::UnknownModel
    for (const ChatModelInfo& m : kChatModels)
        if (std::strcmp(m.cli_name, entry->cli_name) == 0) return &m;
    throw ModelNotFound("Unknown model '" + model_name + "'");
}

// stop_token_ids (models/base.rs:261-271): the first eos id and <|eot_id|> when the tokenizer has it
std::vector<uint32_t> stop_token_ids(const LlmConfig& cfg, const BpeTokenizer& tok)
{
    std::vector<uint32_t> ids;
    if (!cfg.eos_ids.empty()) ids.push_back(cfg.eos_ids[0]);
    uint32_t eot = 0;
    if (tok.token_to_id("<|eot_id|>", eot) && std::find(ids.begin(), ids.end(), eot) == ids.end()) ids.push_back(eot);
    if (ids.empty()) ids.push_back(UINT32_MAX);  // nothing stops generation but the length
    return ids;
}

// DecoderGenerator::encode (generator.rs:141-163): the BOS rule
std::vector<uint32_t> encode_prompt(const BpeTokenizer& tok, const LlmConfig& cfg, const std::string& prompt, const GenerationConfig& config)
{
    std::vector<uint32_t> tokens = tok.encode(prompt);
    if (config.add_bos_token && cfg.has_bos && (tokens.empty() || tokens[0] != cfg.bos_id)) tokens.insert(tokens.begin(), cfg.bos_id);
    return tokens;
}

// The resolved config as the token loop's options (generator.rs:243-246: max_len from max_new_tokens or max_length, capped
// at the model's context).
GenerateOptions text_generation_options(const LlmModel& model, size_t n_tokens, const GenerationConfig& config,
                                        const std::vector<uint32_t>& stop_ids, UniformRng& rng)
{
    const size_t context_size = (size_t)model.config().max_pos;
    GenerateOptions opt;
    opt.max_new_tokens = config.max_new_tokens.has ? config.max_new_tokens.value : (config.max_length > n_tokens ? config.max_length - n_tokens : 0);
    opt.max_len = config.max_new_tokens.has ? n_tokens + config.max_new_tokens.value : config.max_length;
    opt.max_len = std::min(opt.max_len, context_size);
    opt.repetition_penalty = config.repetition_penalty;
    opt.no_repeat_ngram = (int)config.no_repeat_ngram_size;
    opt.stop_ids = stop_ids;
    if (config.strategy == Strategy::Sample) {
        opt.sample = true;
        opt.sampling.temperature = config.temperature;
        opt.sampling.top_k = config.top_k.has ? (int64_t)config.top_k.value : -1;
        opt.sampling.top_p = config.top_p.has ? config.top_p.value : -1.0f;
        opt.sampling.min_p = config.min_p.has ? config.min_p.value : -1.0f;
        opt.uniform = [&rng] { return rng.next(); };
    }
    return opt;
}

// The text side of run_generation_loop shared by Chat and Generator: the resolved config becomes the loop's options, and
// every generated token is decoded on its own, specials kept (generator.rs:343-345), and handed to on_text.
std::string run_text_generation(LlmModel& model, const BpeTokenizer& tok, const std::vector<uint32_t>& tokens, const GenerationConfig& config,
                                const std::vector<uint32_t>& stop_ids, UniformRng& rng, const std::function<bool(const std::string&)>& on_text,
                                int prompt_lookup = 0, int sampled_lookup = 0, LlmModel* drafter = nullptr, int draft_tokens = 0,
                                const DeviceConstraint* constraint = nullptr, ConstraintOutcome* outcome = nullptr,
                                const DeviceGrammar* grammar = nullptr, int logprobs = -1, GeneratedLogprobs* generated = nullptr)
{
    if (tokens.empty()) throw std::runtime_error("generation failed: cannot generate from empty prompt");
    GenerateOptions opt = text_generation_options(model, tokens.size(), config, stop_ids, rng);
    if (generated) *generated = GeneratedLogprobs{};
    const bool records = logprobs >= 0 && generated;
    if (records) {
        opt.logprobs = logprobs;
        opt.logprob_sink = &generated->records;
    }
    opt.constraint = constraint;
    opt.grammar = grammar;
    opt.constraint_outcome = constraint || grammar ? outcome : nullptr;
    std::string text;
    std::vector<uint32_t> prompt_tokens = tokens;
    if ((int)prompt_tokens.size() > model.context()) prompt_tokens.resize((size_t)model.context());
    const auto on_token = [&](uint32_t id) {
        const std::string piece = tok.decode({id}, false);  // one token at a time, specials kept (generator.rs:343-345)
        text += piece;
        if (records) generated->tokens.push_back(id);
        return on_text ? on_text(piece) : true;
    };
    // a draft model (when set) takes precedence over prompt lookup: greedy requests without processors and sampled requests
    // without an n-gram ban verify the drafter's proposals every step; the others take the plain loop inside generate_draft
    // (a constrained request takes the plain loop: the lookup and draft loops do not carry the automaton)
    // (a request that records log-probabilities takes the plain loop too)
    if (constraint || grammar || records) {
        model.generate(prompt_tokens, opt, on_token);
    } else if (drafter && draft_tokens > 0) {
        model.generate_draft(drafter, prompt_tokens, opt, draft_tokens, on_token, nullptr);
    } else if (prompt_lookup > 0 && !opt.sample && opt.repetition_penalty == 1.0f && opt.no_repeat_ngram <= 0) {
        LookupConfig lk;
        lk.draft_tokens = prompt_lookup;
        model.generate_lookup(prompt_tokens, opt, lk, on_token, nullptr);
    } else if (sampled_lookup > 0 && opt.sample && opt.no_repeat_ngram <= 0) {
        // sampled requests (with or without a repetition penalty), when asked for: the same draws decide the same tokens
        LookupConfig lk;
        lk.draft_tokens = sampled_lookup;
        model.generate_lookup_sampled(prompt_tokens, opt, lk, on_token, nullptr);
    } else {
        model.generate(prompt_tokens, opt, on_token);
    }
    return text;
}

}  // namespace

std::unique_ptr<Chat> Chat::create(const std::string& model_name, const std::string& model_dir, const std::string& cache_dir,
                                   const std::string* system_prompt, int mode, bool quiet)
{
    const RegistryEntry* entry = nullptr;
    const ChatModelInfo* info = model_info(model_name, entry);
    const std::string cli = entry->cli_name;
    const std::string family = info->family;
    auto incompatible = [&](const std::string& reason) { return InvalidConfig("model '" + cli + "' is incompatible with chat: " + reason); };
    // validate_for_chat (chat/validation.rs:36-116)
    if (family == "encoder")
        throw incompatible(std::string("Model architecture '") + info->arch +
                           "' is an encoder and cannot generate text. Use an Encoder for embeddings instead.");
    if (family == "whisper")
        throw incompatible(std::string("Model architecture '") + info->arch +
                           "' is designed for speech-to-text transcription. Use a SpeechToText model instead.");
    if (family == "seq2seq")
        throw incompatible(std::string("Model architecture '") + info->arch +
                           "' is a seq2seq model designed for translation/summarization. Use Translator or Summarizer instead.");
    const std::string task = info->task;
    if (task == "generation" && !quiet) std::fprintf(stderr, "Warning: [info] Model '%s' is a base model, not instruction-tuned.\n", cli.c_str());

    const std::string dir = !model_dir.empty() ? model_dir : model_dir_for(*entry, cache_dir.empty() ? default_cache_dir() : cache_dir);
    if (!decoder_files_present(dir))  // DownloadPolicy: this library never downloads
        throw ModelNotFound("model '" + cli + "' not downloaded. run: kjarni model download " + cli);

    auto load_failed = [&](const std::string& why) { return std::runtime_error("failed to load model '" + cli + "': " + why); };
    if (family == "phi3") throw load_failed("Phi3 model loading not yet implemented");
    if (family == "gpt")  // loads in the reference, then fails the template check (chat/model.rs:113-116)
        throw InvalidConfig("model '" + cli + "' does not have a chat template. use Generator for raw text generation.");

    std::unique_ptr<Chat> chat(new Chat());
    chat->model_name_ = cli;
    chat->template_ = (family == "qwen2" || family == "qwen3") ? ChatTemplateKind::ChatML : (family == "mistral" ? ChatTemplateKind::Mistral : ChatTemplateKind::Llama3);
    chat->mode_ = mode;
    if (system_prompt) {
        chat->has_system_ = true;
        chat->system_prompt_ = *system_prompt;
    }
    int device = 0;
    if (const char* dv = std::getenv("KJARNI_HIP_DEVICE")) device = std::atoi(dv);
    int context_cap = 32768;
    if (const char* cv = std::getenv("KJARNI_HIP_CHAT_CONTEXT")) context_cap = std::max(16, std::atoi(cv));
    try {
        chat->tokenizer_.load(dir + "/tokenizer.json");
        chat->model_ = LlmModel::load(dir, device, 0, context_cap);
    } catch (const GpuUnavailable&) {
        throw;
    } catch (const std::exception& e) {
        throw load_failed(e.what());
    }
    const LlmConfig& cfg = chat->model_->config();
    chat->tokenizer_.set_truncation((size_t)cfg.max_pos);  // loader.rs:115-120

    std::string hf;
    const bool has_hf = read_file(dir + "/generation_config.json", hf);
    const GenerationConfig defaults = model_default_generation_config(cfg.model_type, (size_t)cfg.max_pos, has_hf ? &hf : nullptr);
    // Chat::from_builder: the mode supplies temperature and max_new_tokens unless the builder set them (the C ABI never does).
    static const float kModeTemperature[3] = {0.7f, 0.9f, 0.3f};
    static const size_t kModeMaxTokens[3] = {512, 1024, 2048};
    const int m = mode == 1 || mode == 2 ? mode : 0;
    chat->mode_overrides_.temperature = Opt<float>(kModeTemperature[m]);
    chat->mode_overrides_.max_new_tokens = Opt<size_t>(kModeMaxTokens[m]);
    chat->generation_config_ = resolve_generation_config(defaults, chat->mode_overrides_, GenerationOverrides());

    chat->stop_ids_ = stop_token_ids(cfg, chat->tokenizer_);
    return chat;
}

std::vector<ChatMessage> Chat::create_conversation() const
{
    std::vector<ChatMessage> c;
    if (has_system_) c.push_back({ChatRole::System, system_prompt_});
    else if (const char* d = chat_default_system_prompt(template_)) c.push_back({ChatRole::System, d});
    return c;
}

std::vector<ChatMessage> Chat::history_to_conversation(const std::vector<ChatMessage>& history) const
{
    std::vector<ChatMessage> conv;
    bool has_system = false;
    for (const ChatMessage& m : history) {
        if (m.role == ChatRole::System) {  // a system message restarts the conversation (model.rs:157-160)
            conv.clear();
            conv.push_back(m);
            has_system = true;
        } else {
            conv.push_back(m);
        }
    }
    if (!has_system && has_system_) {
        std::vector<ChatMessage> with;
        with.push_back({ChatRole::System, system_prompt_});
        for (const ChatMessage& m : conv)
            if (m.role != ChatRole::System) with.push_back(m);
        return with;
    }
    return conv;
}

GenerationConfig Chat::resolve(const GenerationOverrides& runtime) const
{
    return resolve_generation_config(generation_config_, mode_overrides_, runtime);
}

std::vector<uint32_t> Chat::encode(const std::string& prompt, const GenerationConfig& config) const
{
    return encode_prompt(tokenizer_, model_->config(), prompt, config);
}

// The drafter of a handle: `path` loaded on the target's device with its weights as stored and the target's context, checked
// against the target before it replaces the old one; an empty path or draft_tokens == 0 frees it.
static void set_handle_drafter(LlmModel& target, const std::string& path, int draft_tokens, std::unique_ptr<LlmModel>& drafter, int& tokens)
{
    if (draft_tokens < 0 || draft_tokens > 7) throw InvalidConfig("draft_tokens must be 1..7 (0 = off)");
    if (path.empty() || draft_tokens == 0) {
        drafter.reset();
        tokens = 0;
        return;
    }
    std::unique_ptr<LlmModel> fresh = LlmModel::load(path, target.device(), 0, target.context());
    target.check_draft_pair(fresh.get(), draft_tokens);
    drafter = std::move(fresh);
    tokens = draft_tokens;
}

// The constraint of a handle: `pattern` compiled and its mask built over the model's vocabulary, with the bytes of every token
// from the handle's tokenizer (ids past the tokenizer's own: no bytes); an empty pattern frees it.
static void set_handle_constraint(const LlmModel& model, const BpeTokenizer& tok, const std::string& pattern, std::string& current,
                                  std::unique_ptr<DeviceConstraint>& constraint)
{
    if (pattern.empty()) {
        constraint.reset();
        current.clear();
        return;
    }
    if (constraint && pattern == current) return;
    ConstraintDfa dfa;
    try {
        dfa = compile_constraint(pattern);
    } catch (const ConstraintError& e) {
        throw InvalidConfig(e.what());
    }
    TokenTable table;
    const size_t vocab = (size_t)model.config().vocab;
    table.off.assign(vocab + 1, 0);
    for (size_t t = 0; t < vocab; ++t) {
        const std::string bytes = tok.token_bytes((uint32_t)t);
        table.bytes.insert(table.bytes.end(), bytes.begin(), bytes.end());
        table.off[t + 1] = (uint32_t)table.bytes.size();
    }
    constraint = std::make_unique<DeviceConstraint>(model.device(), std::move(dfa), std::move(table));
    current = pattern;
}

// The grammar of a handle: the rules compiled and placed on the model's device with the same token table; no rule frees it.
static void set_handle_grammar(const LlmModel& model, const BpeTokenizer& tok, const std::vector<std::pair<std::string, std::string>>& rules,
                               std::unique_ptr<DeviceGrammar>& grammar)
{
    if (rules.empty()) {
        grammar.reset();
        return;
    }
    Grammar compiled;
    try {
        compiled = compile_grammar(rules);
    } catch (const GrammarError& e) {
        throw InvalidConfig(e.what());
    }
    TokenTable table;
    const size_t vocab = (size_t)model.config().vocab;
    table.off.assign(vocab + 1, 0);
    for (size_t t = 0; t < vocab; ++t) {
        const std::string bytes = tok.token_bytes((uint32_t)t);
        table.bytes.insert(table.bytes.end(), bytes.begin(), bytes.end());
        table.off[t + 1] = (uint32_t)table.bytes.size();
    }
    grammar = std::make_unique<DeviceGrammar>(model.device(), std::move(compiled), std::move(table));
}

void Chat::set_constraint(const std::string& pattern)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_constraint(*model_, tokenizer_, pattern, constraint_pattern_, constraint_);
    if (constraint_) grammar_.reset();
}

void Generator::set_constraint(const std::string& pattern)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_constraint(*model_, tokenizer_, pattern, constraint_pattern_, constraint_);
    if (constraint_) grammar_.reset();
}

void Chat::set_grammar(const std::vector<std::pair<std::string, std::string>>& rules)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_grammar(*model_, tokenizer_, rules, grammar_);
    if (grammar_) set_handle_constraint(*model_, tokenizer_, "", constraint_pattern_, constraint_);
}

void Generator::set_grammar(const std::vector<std::pair<std::string, std::string>>& rules)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_grammar(*model_, tokenizer_, rules, grammar_);
    if (grammar_) set_handle_constraint(*model_, tokenizer_, "", constraint_pattern_, constraint_);
}

static void check_handle_logprobs(const LlmModel& model, int top_k)
{
    if (top_k < -1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > model.config().vocab)
        throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be -1 (off) or in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                            "] and not above the vocabulary size " + std::to_string(model.config().vocab));
}

void Chat::set_logprobs(int top_k)
{
    std::lock_guard<std::mutex> lock(mutex_);
    check_handle_logprobs(*model_, top_k);
    logprobs_ = top_k;
}

void Generator::set_logprobs(int top_k)
{
    std::lock_guard<std::mutex> lock(mutex_);
    check_handle_logprobs(*model_, top_k);
    logprobs_ = top_k;
}

GeneratedLogprobs Chat::last_logprobs() const
{
    std::lock_guard<std::mutex> lock(mutex_);
    return last_logprobs_;
}

GeneratedLogprobs Generator::last_logprobs(size_t prompt_index) const
{
    std::lock_guard<std::mutex> lock(mutex_);
    return prompt_index < last_logprobs_.size() ? last_logprobs_[prompt_index] : GeneratedLogprobs{};
}

void Chat::set_draft_model(const std::string& path, int draft_tokens)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_drafter(*model_, path, draft_tokens, drafter_, draft_tokens_);
}

void Generator::set_draft_model(const std::string& path, int draft_tokens)
{
    std::lock_guard<std::mutex> lock(mutex_);
    set_handle_drafter(*model_, path, draft_tokens, drafter_, draft_tokens_);
}

std::string Chat::run(const std::string& prompt, const GenerationOverrides& runtime, const std::function<bool(const std::string&)>& on_text)
{
    std::lock_guard<std::mutex> lock(mutex_);
    const GenerationConfig config = resolve(runtime);
    if (config.strategy == Strategy::BeamSearch) throw std::runtime_error("generation failed: Beam search is not supported in this generator.");
    return run_text_generation(*model_, tokenizer_, encode(prompt, config), config, stop_ids_, rng_, on_text, 0,
                               lookup_sampling_ ? LookupConfig().draft_tokens : 0, drafter_.get(), draft_tokens_, constraint_.get(),
                               &constraint_outcome_, grammar_.get(), logprobs_, &last_logprobs_);
}

std::string Chat::generate(const std::string& prompt, const GenerationOverrides& runtime)
{
    std::string cleaned = trim_unicode(run(prompt, runtime, nullptr));
    for (const std::string& stop : chat_stop_sequences(template_))
        if (cleaned.size() >= stop.size() && cleaned.compare(cleaned.size() - stop.size(), stop.size(), stop) == 0)
            cleaned = trim_unicode(cleaned.substr(0, cleaned.size() - stop.size()));
    return cleaned;
}

std::string Chat::generate_stream(const std::string& prompt, const GenerationOverrides& runtime,
                                  const std::function<bool(const std::string&)>& on_text)
{
    return run(prompt, runtime, on_text);
}

// ---- Generator ------------------------------------------------------------------------------------

std::unique_ptr<Generator> Generator::create(const std::string& model_name, const std::string& model_dir, const std::string& cache_dir,
                                             bool quiet)
{
    const RegistryEntry* entry = nullptr;
    const ChatModelInfo* info = model_info(model_name, entry);
    const std::string cli = entry->cli_name;
    const std::string family = info->family;
    // validate_for_generation (generator/validation.rs:8-51)
    auto invalid = [&](const std::string& reason) { return InvalidConfig("Model '" + cli + "' is not suitable for text generation: " + reason); };
    if (family == "encoder")
        throw invalid(std::string("Architecture '") + info->arch + "' is an encoder and cannot generate text. Use Embedder instead.");
    if (family == "whisper") throw invalid("Whisper is designed for speech-to-text. Use Transcriber instead.");
    if (family == "seq2seq")
        throw invalid(std::string("Architecture '") + info->arch +
                      "' is a seq2seq model. Use Seq2SeqGenerator, Translator, or Summarizer instead.");
    if (std::string(info->task) == "generation" && !quiet)
        std::fprintf(stderr, "Warning: [info] Model '%s' is a base model, not instruction-tuned.\n", cli.c_str());

    const std::string dir = !model_dir.empty() ? model_dir : model_dir_for(*entry, cache_dir.empty() ? default_cache_dir() : cache_dir);
    if (!decoder_files_present(dir))  // GeneratorError::ModelNotDownloaded: this library never downloads
        throw ModelNotFound("Model '" + cli + "' not downloaded. Run: kjarni model download " + cli);
    auto load_failed = [&](const std::string& why) { return std::runtime_error("Failed to load model '" + cli + "': " + why); };
    if (family == "phi3") throw load_failed("Phi3 model loading not yet implemented");  // generator/model.rs:222

    std::unique_ptr<Generator> g(new Generator());
    g->model_name_ = cli;
    int device = 0;
    if (const char* dv = std::getenv("KJARNI_HIP_DEVICE")) device = std::atoi(dv);
    int context_cap = 32768;
    if (const char* cv = std::getenv("KJARNI_HIP_CHAT_CONTEXT")) context_cap = std::max(16, std::atoi(cv));
    try {
        g->tokenizer_.load(dir + "/tokenizer.json");
        g->model_ = LlmModel::load(dir, device, 0, context_cap);
    } catch (const GpuUnavailable&) {
        throw;
    } catch (const std::exception& e) {
        throw load_failed(e.what());
    }
    const LlmConfig& cfg = g->model_->config();
    g->tokenizer_.set_truncation((size_t)cfg.max_pos);  // loader.rs:115-120
    std::string hf;
    const bool has_hf = read_file(dir + "/generation_config.json", hf);
    // model.rs:127-132: the model's defaults, resolved with no builder overrides
    g->generation_config_ = resolve_generation_config(
        model_default_generation_config(cfg.model_type, (size_t)cfg.max_pos, has_hf ? &hf : nullptr), GenerationOverrides(), GenerationOverrides());
    g->stop_ids_ = stop_token_ids(cfg, g->tokenizer_);
    return g;
}

GenerationConfig Generator::resolve(const GenerationOverrides& runtime) const
{
    return resolve_generation_config(generation_config_, GenerationOverrides(), runtime);
}

std::vector<uint32_t> Generator::encode(const std::string& prompt, const GenerationConfig& config) const
{
    return encode_prompt(tokenizer_, model_->config(), prompt, config);
}

std::string Generator::run(const std::string& prompt, const GenerationOverrides& runtime, const std::function<bool(const std::string&)>& on_text)
{
    std::lock_guard<std::mutex> lock(mutex_);
    const GenerationConfig config = resolve(runtime);
    if (config.strategy == Strategy::BeamSearch) throw std::runtime_error("generation failed: Beam search is not supported in this generator.");
    last_logprobs_.assign(1, GeneratedLogprobs{});
    return run_text_generation(*model_, tokenizer_, encode(prompt, config), config, stop_ids_, rng_, on_text, prompt_lookup_,
                               lookup_sampling_ ? prompt_lookup_ : 0, drafter_.get(), draft_tokens_, constraint_.get(), &constraint_outcome_,
                               grammar_.get(), logprobs_, &last_logprobs_[0]);
}

size_t Generator::encode_scored(const std::string& context, const std::string& continuation, std::vector<uint32_t>& whole) const
{
    const GenerationConfig config = resolve(GenerationOverrides());
    whole = encode(context + continuation, config);
    const size_t first = encode(context, config).size();
    if (first == 0) throw InvalidConfig("scoring needs at least one context token (the context is empty and the model has no BOS token)");
    if (first >= whole.size())
        throw InvalidConfig("the continuation adds no tokens: context + continuation encode to " + std::to_string(whole.size()) +
                            " tokens, the context alone to " + std::to_string(first));
    if (whole.size() > (size_t)model_->context())
        throw InvalidConfig("context + continuation (" + std::to_string(whole.size()) + " tokens) exceed the model's context of " +
                            std::to_string(model_->context()) + " tokens");
    return first;
}

Generator::Score Generator::score(const std::string& context, const std::string& continuation)
{
    std::lock_guard<std::mutex> lock(mutex_);
    std::vector<uint32_t> whole;
    const size_t first = encode_scored(context, continuation, whole);
    const size_t cnt = whole.size() - first;
    std::vector<float> lp(cnt);
    std::vector<uint32_t> top(cnt);
    model_->score(whole.data(), (int)whole.size(), (int)first, lp.data(), top.data(), nullptr);
    Score r;
    r.n_tokens = cnt;
    r.is_greedy = true;
    for (size_t i = 0; i < cnt; ++i) {
        r.sum_logprob += (double)lp[i];
        if (top[i] != whole[first + i]) r.is_greedy = false;
    }
    return r;
}

std::vector<Generator::Score> Generator::score_batch(const std::vector<std::pair<std::string, std::string>>& pairs)
{
    std::lock_guard<std::mutex> lock(mutex_);
    const size_t n = pairs.size();
    std::vector<std::vector<uint32_t>> whole(n);
    std::vector<size_t> first(n);
    for (size_t i = 0; i < n; ++i) {
        try {
            first[i] = encode_scored(pairs[i].first, pairs[i].second, whole[i]);
        } catch (const InvalidConfig& e) {
            throw InvalidConfig("pair " + std::to_string(i) + ": " + e.what());
        }
    }
    std::vector<Score> out(n);
    auto fill = [&](size_t i, const float* lp, const uint32_t* top) {
        Score& r = out[i];
        r.n_tokens = whole[i].size() - first[i];
        r.is_greedy = true;
        for (size_t t = 0; t < r.n_tokens; ++t) {
            r.sum_logprob += (double)lp[t];
            if (top[t] != whole[i][first[i] + t]) r.is_greedy = false;
        }
    };
    // the packed pairs, in the caller's order
    const bool packed_model = model_->score_batch_supported();
    const size_t limit = (size_t)model_->embed_max_tokens();
    std::vector<size_t> packed;
    std::vector<uint32_t> ids;
    std::vector<int32_t> offsets(1, 0), firsts;
    for (size_t i = 0; i < n; ++i) {
        if (!packed_model || whole[i].size() > limit || ids.size() + whole[i].size() > (size_t)INT32_MAX) continue;
        packed.push_back(i);
        ids.insert(ids.end(), whole[i].begin(), whole[i].end());
        offsets.push_back((int32_t)ids.size());
        firsts.push_back((int32_t)first[i]);
    }
    if (!packed.empty()) {
        size_t total = 0;
        for (size_t i : packed) total += whole[i].size() - first[i];
        std::vector<float> lp(total);
        std::vector<uint32_t> top(total);
        model_->score_batch(ids.data(), offsets.data(), (int)packed.size(), firsts.data(), 1, lp.data(), top.data(), nullptr);
        size_t at = 0;
        for (size_t i : packed) {
            fill(i, lp.data() + at, top.data() + at);
            at += whole[i].size() - first[i];
        }
    }
    size_t next = 0;
    for (size_t i = 0; i < n; ++i) {
        if (next < packed.size() && packed[next] == i) {
            ++next;
            continue;
        }
        const size_t cnt = whole[i].size() - first[i];
        std::vector<float> lp(cnt);
        std::vector<uint32_t> top(cnt);
        model_->score(whole[i].data(), (int)whole[i].size(), (int)first[i], lp.data(), top.data(), nullptr);
        fill(i, lp.data(), top.data());
    }
    return out;
}

Generator::TokenScores Generator::score_tokens(const std::string& context, const std::string& continuation, size_t top_k)
{
    std::lock_guard<std::mutex> lock(mutex_);
    if (top_k < 1 || top_k > (size_t)KJARNI_SCORE_TOPK_MAX || top_k > (size_t)model_->config().vocab)
        throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [1, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                            "] and not above the vocabulary size " + std::to_string(model_->config().vocab));
    std::vector<uint32_t> whole;
    const size_t first = encode_scored(context, continuation, whole);
    const size_t cnt = whole.size() - first;
    TokenScores r;
    r.top_k = top_k;
    r.tokens.assign(whole.begin() + (ptrdiff_t)first, whole.end());
    r.logprobs.resize(cnt);
    r.top_tokens.resize(cnt * top_k);
    r.top_logprobs.resize(cnt * top_k);
    model_->score_topk(whole.data(), (int)whole.size(), (int)first, (int)top_k, r.logprobs.data(), r.top_tokens.data(), r.top_logprobs.data());
    return r;
}

// Generator::run for every prompt, `lanes` of them decoded in lock step (LlmModel::generate_lanes): each prompt is encoded
// (BOS rule), capped and decoded exactly as run() does.  A sampled request draws from a generator of its own, seeded from
// the handle's at call start -- one draw per request, in request order -- so a seeded batch does not depend on the lane count.
std::vector<std::string> Generator::generate_batch(const std::vector<std::string>& prompts, const GenerationOverrides& runtime, int lanes)
{
    std::lock_guard<std::mutex> lock(mutex_);
    const GenerationConfig config = resolve(runtime);
    if (config.strategy == Strategy::BeamSearch) throw std::runtime_error("generation failed: Beam search is not supported in this generator.");
    std::vector<UniformRng> rngs;
    rngs.reserve(prompts.size());
    std::vector<LaneRequest> reqs(prompts.size());
    last_logprobs_.assign(prompts.size(), GeneratedLogprobs{});
    // the handle's pattern or grammar (it holds at most one) constrains every prompt on its lane
    batch_kind_ = constraint_ ? 1 : grammar_ ? 2 : 0;
    batch_outcomes_.assign(batch_kind_ ? prompts.size() : 0, ConstraintOutcome{});
    batch_seeds_.clear();
    for (size_t i = 0; i < prompts.size(); ++i) {
        const uint64_t seed = config.strategy == Strategy::Sample ? (uint64_t)(rng_.next() * 16777216.0f) + 1 : 1;
        rngs.emplace_back(seed);
        batch_seeds_.push_back(seed);
        std::vector<uint32_t> tokens = encode(prompts[i], config);
        if (tokens.empty()) throw std::runtime_error("generation failed: cannot generate from empty prompt (prompt " + std::to_string(i) + ")");
        reqs[i].options = text_generation_options(*model_, tokens.size(), config, stop_ids_, rngs[i]);
        if (logprobs_ >= 0) {
            reqs[i].options.logprobs = logprobs_;
            reqs[i].options.logprob_sink = &last_logprobs_[i].records;
        }
        if (batch_kind_) {
            reqs[i].options.constraint = constraint_.get();
            reqs[i].options.grammar = grammar_.get();
            reqs[i].options.constraint_outcome = &batch_outcomes_[i];
        }
        if ((int)tokens.size() > model_->context()) tokens.resize((size_t)model_->context());
        reqs[i].prompt = std::move(tokens);
    }
    std::vector<std::string> texts(prompts.size());
    const std::function<bool(size_t, uint32_t)> on_token = [&](size_t r, uint32_t id) {
        texts[r] += tokenizer_.decode({id}, false);  // one token at a time, specials kept (generator.rs:343-345)
        if (logprobs_ >= 0) last_logprobs_[r].tokens.push_back(id);
        return true;
    };
    if (wide_lanes_ > 0) model_->generate_wide(reqs, wide_lanes_, 0, on_token);  // (set_wide_lanes: up to 64, the wide step above 8)
    else model_->generate_lanes(reqs, lanes, 0, on_token);
    return texts;
}

uint64_t Generator::batch_seed(size_t prompt_index) const
{
    std::lock_guard<std::mutex> lock(mutex_);
    return prompt_index < batch_seeds_.size() ? batch_seeds_[prompt_index] : 0;
}

ConstraintOutcome Generator::batch_constraint_outcome(size_t prompt_index, int* kind) const
{
    std::lock_guard<std::mutex> lock(mutex_);
    const bool have = prompt_index < batch_outcomes_.size();
    if (kind) *kind = have ? batch_kind_ : 0;
    return have ? batch_outcomes_[prompt_index] : ConstraintOutcome{};
}

}  // namespace kjarni
