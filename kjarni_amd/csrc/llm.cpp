#include "host_util.h"
#include "llm.h"
#include "ffi_common.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>

#include "fp8_weights.h"
#include "gguf.h"
#include "json.h"
#include "kernels.h"
#include "decoder_embed_kernels.h"
#include "draft_model_kernels.h"
#include "llm_kernels.h"
#include "moe_kernels.h"
#include "constraint_kernels.h"
#include "grammar_kernels.h"
#include "lane_constraint_kernels.h"
#include "logprob_kernels.h"
#include "score_batch_kernels.h"
#include "answer_logits_kernels.h"
#include "safetensors.h"
#include "whisper_kernels.h"

namespace kjarni {

namespace {

uint16_t f32_to_bf16(float v)  // round to nearest even
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

}  // namespace

LlmConfig LlmConfig::from_json(const std::string& text)
{
    const Json j = Json::parse(text);
    LlmConfig c;
    auto req = [&](const char* k) {
        const Json* v = j.find(k);
        if (!v || !v->is_number()) throw std::runtime_error(std::string("config.json: missing field `") + k + "`");
        return (int)v->as_int();
    };
    c.model_type = j.get_string("model_type", "llama");
    if (c.model_type != "llama" && c.model_type != "qwen2" && c.model_type != "qwen3" && c.model_type != "qwen3_moe" && c.model_type != "mistral" &&
        c.model_type != "gpt2")
        throw std::runtime_error("unsupported decoder model_type '" + c.model_type + "' (llama, qwen2, qwen3, qwen3_moe, mistral and gpt2 are)");
    auto ids = [&] {  // eos / bos as for every type
        if (const Json* e = j.find("eos_token_id")) {
            if (e->is_number()) c.eos_ids.push_back((uint32_t)e->as_int());
            else if (e->is_array())
                for (const Json& x : e->arr)
                    if (x.is_number()) c.eos_ids.push_back((uint32_t)x.as_int());
        }
        if (const Json* b = j.find("bos_token_id"); b && b->is_number()) {
            c.has_bos = true;
            c.bos_id = (uint32_t)b->as_int();
        }
    };
    if (c.gpt2()) {  // gpt2/config.rs:8-105, HF field names
        c.hidden = req("n_embd");
        c.layers = req("n_layer");
        c.heads = c.kv_heads = req("n_head");
        c.max_pos = req("n_ctx");  // what the reference reads; HF files also carry n_positions, which must agree
        if (const Json* np = j.find("n_positions"); np && np->is_number() && (int)np->as_int() != c.max_pos)
            throw std::runtime_error("config.json: n_positions (" + std::to_string(np->as_int()) + ") differs from n_ctx (" +
                                     std::to_string(c.max_pos) + ")");
        c.vocab = req("vocab_size");
        if (c.heads <= 0 || c.hidden % c.heads) throw std::runtime_error("config.json: unsupported head geometry");
        c.head_dim = c.hidden / c.heads;
        c.eps = (float)j.get_double("layer_norm_epsilon", 1e-5);
        c.tie_embeddings = true;  // the head is wte
        // activations.rs:40-41: gelu, gelu_new and gelu_fast all run the tanh form, as does an absent field
        if (const Json* a = j.find("activation_function"); a && !a->is_null()) {
            const std::string act = a->is_string() ? a->str : std::string("?");
            if (act != "gelu_new" && act != "gelu_fast" && act != "gelu")
                throw std::runtime_error("config.json: unsupported activation_function '" + act + "' (gelu_new, gelu_fast and gelu are)");
        }
        const Json* ni = j.find("n_inner");  // cpu_decoder.rs:194; the loader checks it against the c_fc weight
        c.inter = ni && ni->is_number() ? (int)ni->as_int() : 4 * c.hidden;
        c.rope_theta = 0.0f;
        ids();
        return c;
    }
    c.hidden = req("hidden_size");
    c.layers = req("num_hidden_layers");
    c.heads = req("num_attention_heads");
    c.kv_heads = (int)j.get_int("num_key_value_heads", c.heads);
    c.inter = req("intermediate_size");
    c.vocab = req("vocab_size");
    c.max_pos = req("max_position_embeddings");
    c.head_dim = (int)j.get_int("head_dim", c.hidden / c.heads);
    // llama/config.rs:137-152, qwen/config.rs:70-76, mistral/config.rs:54-56 + :168 defaults.  Mistral runs on the Llama
    // decoder (mistral/model.rs:56-62); its sliding_window field is never read by the reference.
    const bool llama = c.model_type == "llama", mistral = c.model_type == "mistral";
    c.eps = (float)j.get_double("rms_norm_eps", (llama || mistral) ? 1e-5 : 1e-6);
    c.rope_theta = (float)j.get_double("rope_theta", llama ? 500000.0 : (mistral ? 10000.0 : 1000000.0));
    c.tie_embeddings = j.get_bool("tie_word_embeddings", llama);
    if (const Json* rs = j.find("rope_scaling"); rs && rs->is_object()) {
        c.has_rope_scaling = true;
        c.rope_type = rs->get_string("rope_type", rs->get_string("type", ""));
        c.rope_factor = (float)rs->get_double("factor", 1.0);
        c.rope_low = (float)rs->get_double("low_freq_factor", 1.0);
        c.rope_high = (float)rs->get_double("high_freq_factor", 4.0);
        c.rope_original_max = (int)rs->get_int("original_max_position_embeddings", 8192);
    }
    ids();
    if (c.moe()) {  // (HF Qwen3MoeConfig: norm_topk_prob defaults to false, decoder_sparse_step to 1, mlp_only_layers to [])
        c.num_experts = req("num_experts");
        c.experts_per_tok = req("num_experts_per_tok");
        c.moe_inter = req("moe_intermediate_size");
        c.norm_topk = j.get_bool("norm_topk_prob", false);
        c.sparse_step = (int)j.get_int("decoder_sparse_step", 1);
        if (const Json* ml = j.find("mlp_only_layers"); ml && ml->is_array())
            for (const Json& x : ml->arr)
                if (x.is_number()) c.mlp_only_layers.push_back((int)x.as_int());
        if (c.num_experts < 2 || c.num_experts > 256)
            throw std::runtime_error("config.json: num_experts is " + std::to_string(c.num_experts) + "; 2 .. 256 are supported");
        if (c.experts_per_tok < 1 || c.experts_per_tok > 8 || c.experts_per_tok > c.num_experts)
            throw std::runtime_error("config.json: num_experts_per_tok is " + std::to_string(c.experts_per_tok) + " with num_experts " +
                                     std::to_string(c.num_experts) + "; 1 .. 8 and at most num_experts are supported");
        if (c.moe_inter < 32 || c.moe_inter % 32)
            throw std::runtime_error("config.json: moe_intermediate_size is " + std::to_string(c.moe_inter) + "; a positive multiple of 32 is needed");
        if (c.sparse_step < 1) throw std::runtime_error("config.json: decoder_sparse_step is " + std::to_string(c.sparse_step) + "; it must be at least 1");
        if (j.find("quantization_config"))
            throw std::runtime_error("config.json: a qwen3_moe checkpoint with a quantization_config: quantized mixture-of-experts checkpoints "
                                     "(FP8, GGUF) are out of scope, bf16 and f32 are supported");
    }
    // Qwen3 sets head_dim apart from hidden / heads (0.6B: 16 heads x 128 over a hidden size of 1024); the others may not
    if (c.heads <= 0 || c.kv_heads <= 0 || c.heads % c.kv_heads != 0 || c.head_dim <= 0 || (!c.qwen3() && c.head_dim * c.heads != c.hidden))
        throw std::runtime_error("config.json: unsupported head geometry");
    return c;
}

bool LlmConfig::sparse_layer(int i) const
{
    if (num_experts <= 0 || sparse_step < 1) return false;
    if (std::find(mlp_only_layers.begin(), mlp_only_layers.end(), i) != mlp_only_layers.end()) return false;
    return (i + 1) % sparse_step == 0;
}

// Everything about a qwen3_moe directory that can be refused without a device: the config (from_json), then per layer the
// tensors its kind needs, by name and shape.  A sparse layer: mlp.gate.weight [E, hidden] and, per expert, gate_proj / up_proj
// [Im, hidden] and down_proj [hidden, Im], and no dense mlp.gate_proj beside them; a dense layer: the three Qwen3 matrices.
void LlmModel::check_moe_checkpoint(const std::string& dir)
{
    std::string text;
    {
        std::ifstream f(dir + "/config.json", std::ios::binary);
        if (!f) return;  // a .gguf file (its reader refuses the qwen3moe architecture by name) or nothing load() can read
        text.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    }
    try {
        if (Json::parse(text).get_string("model_type", "llama") != "qwen3_moe") return;
    } catch (const std::exception&) {
        return;
    }
    const LlmConfig c = LlmConfig::from_json(text);
    const int H = c.hidden, E = c.num_experts, Im = c.moe_inter;
    if (H % 32 || H > 8192) throw std::runtime_error("qwen3_moe: hidden_size is " + std::to_string(H) + "; a multiple of 32 up to 8192 is needed");
    if ((int64_t)c.experts_per_tok * Im > 16384)
        throw std::runtime_error("qwen3_moe: num_experts_per_tok * moe_intermediate_size is " + std::to_string((int64_t)c.experts_per_tok * Im) +
                                 "; at most 16384 is supported");
    SafeTensors st;
    if (!resolve_gguf(dir).empty())  // (no safetensors beside the config, a .gguf file instead)
        throw std::runtime_error("GGUF qwen3_moe checkpoint: quantized mixture-of-experts checkpoints (FP8, GGUF) are out of scope; bf16 and f32 "
                                 "safetensors are supported");
    st.open_dir(dir);
    auto shape_text = [](const std::vector<int64_t>& s) {
        std::string t = "[";
        for (size_t i = 0; i < s.size(); ++i) t += (i ? ", " : "") + std::to_string(s[i]);
        return t + "]";
    };
    auto need = [&](const std::string& name, std::vector<int64_t> want) {
        if (!st.contains(name)) throw std::runtime_error("missing tensor " + name);
        const TensorView& t = st.get(name);
        if (t.dtype != "F32" && t.dtype != "F16" && t.dtype != "BF16")
            throw std::runtime_error("tensor " + name + " is " + t.dtype + ": a qwen3_moe checkpoint holds F32, F16 or BF16 tensors; quantized "
                                     "mixture-of-experts checkpoints (FP8, GGUF) are out of scope");
        if (t.shape != want) throw std::runtime_error("tensor " + name + " has shape " + shape_text(t.shape) + ", expected " + shape_text(want));
    };
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".mlp.";
        if (!c.sparse_layer(i)) {
            need(p + "gate_proj.weight", {c.inter, H});
            need(p + "up_proj.weight", {c.inter, H});
            need(p + "down_proj.weight", {H, c.inter});
            continue;
        }
        if (st.contains(p + "gate_proj.weight"))
            throw std::runtime_error("sparse layer " + std::to_string(i) + " also carries the dense tensor " + p + "gate_proj.weight");
        need(p + "gate.weight", {E, H});
        for (int e = 0; e < E; ++e) {
            const std::string q = p + "experts." + std::to_string(e) + ".";
            need(q + "gate_proj.weight", {Im, H});
            need(q + "up_proj.weight", {Im, H});
            need(q + "down_proj.weight", {H, Im});
        }
    }
}

float* LlmModel::dalloc(size_t floats)
{
    return static_cast<float*>(arena_.alloc(std::max<size_t>(floats, 4) * sizeof(float)));   // (device_arena.h: blocks, not one hipMalloc per tensor)
}

float* LlmModel::upload_f32(const std::vector<float>& host)
{
    float* d = dalloc(host.size());
    if (!host.empty()) hip_check(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(weights)");
    weight_bytes_ += host.size() * sizeof(float);
    bytes_by_type_[GGML_F32] += host.size() * sizeof(float);
    return d;
}

void* LlmModel::upload_weight(const std::vector<float>& host)
{
    if (!bf16_) return upload_f32(host);
    std::vector<uint16_t> h(host.size());
    for (size_t i = 0; i < host.size(); ++i) h[i] = f32_to_bf16(host[i]);  // exact when the file already held bf16
    void* d = dalloc((host.size() + 1) / 2);
    if (!h.empty()) hip_check(hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice), "hipMemcpy(weights)");
    weight_bytes_ += h.size() * 2;
    bytes_by_type_[GGML_BF16] += h.size() * 2;
    return d;
}

LlmModel::~LlmModel()
{
    if (host_logits_) (void)hipHostFree(host_logits_);
    if (emeta_host_) (void)hipHostFree(emeta_host_);
    if (sb_res_host_) (void)hipHostFree(sb_res_host_);
    if (samp_host_) (void)hipHostFree(samp_host_);
    if (ls_host_) (void)hipHostFree(ls_host_);
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (graph_) (void)hipGraphExecDestroy(graph_);
    if (cgraph_) (void)hipGraphExecDestroy(cgraph_);
    if (ggraph_) (void)hipGraphExecDestroy(ggraph_);
    for (auto& kind : lp_graphs_)
        for (hipGraphExec_t& g : kind)
            if (g) (void)hipGraphExecDestroy(g);
    drop_lane_graphs(lane_bank_);
    drop_lane_graphs(wide_bank_);
    drop_graphs(lookup_graphs_);
    drop_graphs(lookup_sampled_graphs_);
    if (stream_) (void)hipStreamDestroy(stream_);
    arena_.release();
}

std::unique_ptr<LlmModel> LlmModel::load(const std::string& dir, int device, int weights, int max_context)
{
    check_moe_checkpoint(dir);  // (returns at once for every other kind of checkpoint)
    if (visible_device_count() <= device) throw GpuUnavailable("no usable HIP device " + std::to_string(device));
    std::unique_ptr<LlmModel> m(new LlmModel());
    m->device_ = device;
    static std::atomic<uint64_t> next_serial{1};  // (0 is "no drafter" in the graph keys)
    m->serial_ = next_serial.fetch_add(1);
    hip_check(hipSetDevice(device), "hipSetDevice");
    // a `.gguf` file, or a directory: safetensors win, else its first `*.gguf` (model_weights.rs:45-77)
    const std::string gguf_path = resolve_gguf(dir);
    const bool is_gguf = !gguf_path.empty();
    GgufFile gf;
    SafeTensors st;
    if (is_gguf) {
        gf.open(gguf_path);
        m->config_json_ = gf.config_json();
    } else {
        m->config_json_ = slurp(dir + "/config.json");
    }
    m->cfg_ = LlmConfig::from_json(m->config_json_);
    const LlmConfig& c = m->cfg_;
    const int H = c.hidden, d = c.head_dim, kv = c.kv_heads * d, QD = c.q_dim();
    if ((d & 3) || d > 128 || 256 % (d / 4) != 0 || (H & 7) || (c.inter & 7)) throw std::runtime_error("unsupported decoder geometry");
    auto contains = [&](const std::string& name) { return is_gguf ? gf.find_hf(name) != nullptr : st.contains(name); };
    if (is_gguf) {
        // every matrix must be Q8_0 / Q4_K / Q6_K (the reference's F16 LinearLayer is unimplemented; F32 is for norms and biases)
        std::vector<std::string> mats = {"model.embed_tokens.weight"};
        if (contains("lm_head.weight")) mats.push_back("lm_head.weight");
        for (int i = 0; i < c.layers; ++i)
            for (const char* nm : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                                   "mlp.down_proj"})
                mats.push_back("model.layers." + std::to_string(i) + "." + nm + ".weight");
        for (const std::string& nm : mats) {
            const GgufTensor* t = gf.find_hf(nm);
            if (t && !ggml_matrix_type(t->type))
                throw std::runtime_error("GGUF: matrix " + t->name + " has unsupported type " + ggml_type_name(t->type) + " (" +
                                         std::to_string(t->type) + "); Q8_0, Q4_K and Q6_K are supported");
        }
        m->bf16_ = weights == 2;
        m->quant_ = weights == 0;
    } else {
        st.open_dir(dir);
        if (c.gpt2()) {
            m->cache_cap_ = std::min(max_context > 0 ? max_context : c.max_pos, c.max_pos);
            m->load_gpt2(st, weights);
            m->finish_load();
            return m;
        }
        m->bf16_ = weights == 2 || (weights == 0 && st.get("model.layers.0.self_attn.q_proj.weight").dtype == "BF16");
    }
    // FP8 checkpoints (fp8_weights.h): as stored, the seven matrices of every layer stay FP8 codes in HBM -- all of them or none
    const Fp8Checkpoint f8(st, is_gguf ? std::string() : m->config_json_);
    if (!is_gguf && weights == 0) {
        std::string first_fp8, first_other, other_dtype;
        for (int i = 0; i < c.layers; ++i)
            for (const char* nm : {"self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                                   "mlp.down_proj"}) {
                const std::string name = "model.layers." + std::to_string(i) + "." + nm + ".weight";
                if (f8.is_fp8(name)) {
                    if (first_fp8.empty()) first_fp8 = name;
                } else if (first_other.empty() && st.contains(name)) {
                    first_other = name;
                    other_dtype = st.get(name).dtype;
                }
            }
        if (!first_fp8.empty() && !first_other.empty())
            throw std::runtime_error("mixed FP8 checkpoint: " + first_other + " is " + other_dtype + " while " + first_fp8 +
                                     " is F8_E4M3; weights_dtype 0 keeps FP8 layers only when all seven matrices of every layer are FP8 "
                                     "(weights_dtype 1 or 2 loads the file)");
        if (!first_fp8.empty()) {
            m->quant_ = m->fp8_ = true;
            m->bf16_ = st.get("model.embed_tokens.weight").dtype == "BF16";  // the table and the head stay as stored
        }
    }
    std::vector<float> buf, tmp;
    auto read = [&](const std::string& name, std::vector<float>& out) {
        if (is_gguf) return gf.read_f32(name, out);
        return f8.is_fp8(name) ? f8.read_f32(name, out) : st.read_f32(name, out);
    };
    auto get = [&](const std::string& name, std::vector<int64_t> want) {
        const std::vector<int64_t> shape = read(name, buf);
        if (shape != want) throw std::runtime_error("tensor " + name + " has an unexpected shape");
    };
    // a quantized matrix [n, k]: HF row order, repacked into its device planes (quant_kernels.hip)
    auto upload_q = [&](const std::string& name, int n, int k) {
        const GgufTensor& t = gf.get_hf(name);
        if (t.ne.size() != 2 || t.ne[0] != k || t.ne[1] != n) throw std::runtime_error("tensor " + name + " has an unexpected shape");
        const std::vector<uint8_t> raw = gf.rows_hf(name);
        const QPlanes planes = repack_ggml(t.type, raw.data(), n, k);
        const void* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 4; ++i) {
            const std::vector<uint8_t>& pl = planes.plane[i];
            if (pl.empty()) continue;
            void* dp = m->dalloc((pl.size() + 3) / 4);
            hip_check(hipMemcpy(dp, pl.data(), pl.size(), hipMemcpyHostToDevice), "hipMemcpy(weights)");
            m->weight_bytes_ += pl.size();
            m->bytes_by_type_[t.type] += pl.size();
            ptr[i] = dp;
        }
        QMat q;
        q.type = t.type;
        q.n = n;
        q.k = k;
        q.q = ptr[0];
        q.q2 = ptr[1];
        q.s = ptr[2];
        q.s2 = ptr[3];
        return q;
    };
    // an FP8 matrix [n, k]: the codes as they are in the file, the scales widened to f32 (counted as F32)
    auto upload_f8 = [&](const std::string& name, int n, int k) {
        const Fp8Tensor t = f8.read(name);
        if (t.n != n || t.k != k) throw std::runtime_error("tensor " + name + " has an unexpected shape");
        const size_t bytes = (size_t)n * k;
        void* dp = m->dalloc((bytes + 3) / 4);
        hip_check(hipMemcpy(dp, t.codes, bytes, hipMemcpyHostToDevice), "hipMemcpy(weights)");
        m->weight_bytes_ += bytes;
        m->bytes_by_type_[kFp8WeightType] += bytes;
        Fp8Mat f;
        f.n = n;
        f.k = k;
        f.codes = static_cast<const uint8_t*>(dp);
        f.scale = m->upload_f32(t.scale);
        f.kind = t.kind;
        return f;
    };
    if (m->quant_ && !m->fp8_ && (H % 256 || c.inter % 256)) throw std::runtime_error("quantized GGUF decoder needs hidden and intermediate sizes that are multiples of 256");
    m->layers_.resize((size_t)c.layers);
    m->cache_cap_ = std::min(max_context > 0 ? max_context : c.max_pos, c.max_pos);
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "model.layers." + std::to_string(i);
        Layer& L = m->layers_[(size_t)i];
        L.wqkv = L.wo = L.gate = L.up = L.down = nullptr;
        std::vector<float> w, b;
        bool any_bias = false;
        for (const auto& nm : {std::make_pair(std::string("q_proj"), QD), std::make_pair(std::string("k_proj"), kv),
                               std::make_pair(std::string("v_proj"), kv)}) {
            if (m->fp8_) {
                Fp8Mat& f = nm.first == "q_proj" ? L.fq : (nm.first == "k_proj" ? L.fk : L.fv);
                f = upload_f8(p + ".self_attn." + nm.first + ".weight", nm.second, H);
            } else if (m->quant_) {
                QMat& q = nm.first == "q_proj" ? L.q : (nm.first == "k_proj" ? L.k : L.v);
                q = upload_q(p + ".self_attn." + nm.first + ".weight", nm.second, H);
            } else {
                get(p + ".self_attn." + nm.first + ".weight", {nm.second, H});
                w.insert(w.end(), buf.begin(), buf.end());
            }
            if (contains(p + ".self_attn." + nm.first + ".bias")) {  // Qwen2 (qwen/config.rs:228-234)
                read(p + ".self_attn." + nm.first + ".bias", tmp);
                if ((int)tmp.size() != nm.second) throw std::runtime_error("tensor " + p + ".self_attn." + nm.first + ".bias has an unexpected shape");
                b.insert(b.end(), tmp.begin(), tmp.end());
                any_bias = true;
            } else {
                b.insert(b.end(), (size_t)nm.second, 0.0f);
            }
        }
        L.bqkv = any_bias ? m->upload_f32(b) : nullptr;
        if (m->fp8_) {
            L.fo = upload_f8(p + ".self_attn.o_proj.weight", H, QD);
            L.fgate = upload_f8(p + ".mlp.gate_proj.weight", c.inter, H);
            L.fup = upload_f8(p + ".mlp.up_proj.weight", c.inter, H);
            L.fdown = upload_f8(p + ".mlp.down_proj.weight", H, c.inter);
        } else if (m->quant_) {
            L.o = upload_q(p + ".self_attn.o_proj.weight", H, H);
            L.gate_q = upload_q(p + ".mlp.gate_proj.weight", c.inter, H);
            L.up_q = upload_q(p + ".mlp.up_proj.weight", c.inter, H);
            L.down_q = upload_q(p + ".mlp.down_proj.weight", H, c.inter);
        } else {
            L.wqkv = m->upload_weight(w);
            get(p + ".self_attn.o_proj.weight", {H, QD});
            L.wo = m->upload_weight(buf);
            if (c.sparse_layer(i)) {
                // the router and the three expert stacks in the weights' dtype, each expert uploaded into its place in a
                // preallocated stack (no host copy of a whole stack: 128 experts of the 30B model are 1.2 GB per layer)
                const int E = c.num_experts, Im = c.moe_inter;
                L.moe = true;
                get(p + ".mlp.gate.weight", {E, H});
                L.router = m->upload_weight(buf);
                const size_t per = (size_t)Im * H, wsz = m->bf16_ ? 2 : 4;
                void* stacks[3];
                for (void*& sp : stacks) sp = m->dalloc(((size_t)E * per * wsz + 3) / 4);
                std::vector<uint16_t> half;
                for (int e = 0; e < E; ++e) {
                    const std::string q = p + ".mlp.experts." + std::to_string(e) + ".";
                    const char* names[3] = {"gate_proj.weight", "up_proj.weight", "down_proj.weight"};
                    for (int t = 0; t < 3; ++t) {
                        if (!contains(q + names[t])) throw std::runtime_error("missing tensor " + q + names[t]);
                        get(q + names[t], t == 2 ? std::vector<int64_t>{H, Im} : std::vector<int64_t>{Im, H});
                        const void* src = buf.data();
                        if (m->bf16_) {
                            half.resize(per);
                            for (size_t x = 0; x < per; ++x) half[x] = f32_to_bf16(buf[x]);  // exact when the file already held bf16
                            src = half.data();
                        }
                        hip_check(hipMemcpy(static_cast<char*>(stacks[t]) + (size_t)e * per * wsz, src, per * wsz, hipMemcpyHostToDevice),
                                  "hipMemcpy(expert)");
                    }
                }
                m->weight_bytes_ += 3 * (size_t)E * per * wsz;
                m->bytes_by_type_[m->bf16_ ? GGML_BF16 : GGML_F32] += 3 * (uint64_t)E * per * wsz;
                L.gate_stack = stacks[0];
                L.up_stack = stacks[1];
                L.down_stack = stacks[2];
                L.moe_ids = reinterpret_cast<int32_t*>(m->dalloc((size_t)kMoeRecordRows * c.experts_per_tok));
                L.moe_weights = m->dalloc((size_t)kMoeRecordRows * c.experts_per_tok);
            } else {
                get(p + ".mlp.gate_proj.weight", {c.inter, H});
                L.gate = m->upload_weight(buf);
                get(p + ".mlp.up_proj.weight", {c.inter, H});
                L.up = m->upload_weight(buf);
                get(p + ".mlp.down_proj.weight", {H, c.inter});
                L.down = m->upload_weight(buf);
            }
        }
        get(p + ".input_layernorm.weight", {H});
        L.ln1 = m->upload_f32(buf);
        get(p + ".post_attention_layernorm.weight", {H});
        L.ln2 = m->upload_f32(buf);
        if (c.qwen3()) {  // per-head RMSNorm weights of Q and K, [head_dim] each
            for (const char* nm : {"q_norm", "k_norm"}) {
                const std::string name = p + ".self_attn." + nm + ".weight";
                if (!contains(name)) throw std::runtime_error("missing tensor " + name);
                get(name, {d});
                (nm[0] == 'q' ? L.q_norm : L.k_norm) = m->upload_f32(buf);
            }
        }
        L.k_cache = m->dalloc((size_t)m->cache_cap_ * kv);
        L.v_cache = m->dalloc((size_t)m->cache_cap_ * kv);
    }
    const bool tied = c.tie_embeddings || !contains("lm_head.weight");
    if (m->quant_ && !m->fp8_) {
        m->qembed_ = upload_q("model.embed_tokens.weight", c.vocab, H);
        m->qhead_ = tied ? m->qembed_ : upload_q("lm_head.weight", c.vocab, H);
        m->head_q8k_ = !tied;  // a tied head is the embedding table: dequantized rows x f32 activations (cpu/embeddings/mod.rs:94-132)
    } else {
        get("model.embed_tokens.weight", {c.vocab, H});
        m->embed_ = m->upload_weight(buf);
        if (tied) {
            m->lm_head_ = m->embed_;
        } else {
            get("lm_head.weight", {c.vocab, H});
            m->lm_head_ = m->upload_weight(buf);
        }
    }
    get("model.norm.weight", {H});
    m->final_norm_ = m->upload_f32(buf);
    // llama.cpp files carry llama3 RoPE scaling as per-frequency divisors (rope_freqs.weight); the reference ignores them
    std::vector<float> rope_freqs;
    if (is_gguf && gf.find_hf("rope_freqs.weight")) {
        read("rope_freqs.weight", rope_freqs);
        if ((int)rope_freqs.size() != d / 2) throw std::runtime_error("tensor rope_freqs.weight has an unexpected shape");
    }

    // RoPE tables as the reference builds them (rope/mod.rs:62-130), [cache_cap, d/2]
    {
        const int half = d / 2;
        std::vector<float> inv((size_t)half);
        for (int i = 0; i < half; ++i) inv[(size_t)i] = 1.0f / std::pow(c.rope_theta, (float)(2 * i) / (float)d);
        if (!rope_freqs.empty()) {
            for (int i = 0; i < half; ++i) inv[(size_t)i] = inv[(size_t)i] / rope_freqs[(size_t)i];
        } else if (c.has_rope_scaling && c.rope_type == "llama3") {
            const float low_wl = (float)c.rope_original_max / c.rope_low, high_wl = (float)c.rope_original_max / c.rope_high;
            for (int i = 0; i < half; ++i) {
                const float base = inv[(size_t)i];
                const float wl = 2.0f * (float)M_PI / base;
                if (wl < high_wl) continue;
                if (wl > low_wl) {
                    inv[(size_t)i] = base / c.rope_factor;
                } else {
                    const float smooth = ((float)c.rope_original_max / wl - c.rope_low) / (c.rope_high - c.rope_low);
                    inv[(size_t)i] = base / ((1.0f - smooth) * c.rope_factor + smooth);
                }
            }
        }
        std::vector<float> cs((size_t)m->cache_cap_ * half), sn((size_t)m->cache_cap_ * half);
        for (int p = 0; p < m->cache_cap_; ++p)
            for (int i = 0; i < half; ++i) {
                const float angle = (float)p * inv[(size_t)i];
                cs[(size_t)p * half + i] = std::cos(angle);
                sn[(size_t)p * half + i] = std::sin(angle);
            }
        m->cos_ = m->upload_f32(cs);
        m->sin_ = m->upload_f32(sn);
    }
    m->finish_load();
    return m;
}

void LlmModel::finish_load()
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden, d = c.head_dim, QD = c.q_dim();
    // key ranges per head: up to 512 keys each (128 of them are one register-held pass of the attention kernel); few enough
    // that the output projection can merge the slabs itself
    splits_ = std::max(1, std::min(64, (cache_cap_ + 511) / 512));
    while ((cache_cap_ + splits_ - 1) / splits_ > 512) ++splits_;
    h_ = dalloc(8 * (size_t)H);
    q_ = dalloc(8 * (size_t)QD);
    ctx_ = dalloc(8 * (size_t)QD);
    last_ = dalloc(8 * (size_t)H);
    mid_ = dalloc(8 * (size_t)c.inter);
    if (quant_) {
        const size_t wide = (size_t)std::max(H, c.inter);
        xn_ = dalloc(8 * wide);
        xq_ = reinterpret_cast<int8_t*>(dalloc(2 * wide));
        xd_ = dalloc(8 * wide / 256 + 4);
    }
    if (c.moe()) {
        moe_logits_ = dalloc(8 * (size_t)c.num_experts);
        moe_mid_ = dalloc(8 * (size_t)c.experts_per_tok * c.moe_inter);
    }
    logits_ = dalloc((size_t)c.vocab);
    att_scratch_ = dalloc(decode_attention_scratch_floats(8, c.heads, d, splits_));
    ids_ = reinterpret_cast<uint32_t*>(dalloc(8));
    token_ = reinterpret_cast<int32_t*>(dalloc(4));
    hist_cap_ = cache_cap_ + 16;
    hist_ = reinterpret_cast<int32_t*>(dalloc((size_t)hist_cap_));
    pos_ = reinterpret_cast<int*>(dalloc(4));
    count_ = reinterpret_cast<int*>(dalloc(4));
    best_ = reinterpret_cast<unsigned long long*>(dalloc(4));
    hip_check(hipMemset(best_, 0, 8), "memset");
    hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize(load)");
}

// GPT-2 tensors (gpt2/config.rs:80-125).  gpt2 files name them `wte.weight`, `h.0.attn.c_attn.weight`, ...; distilgpt2 files
// carry a `transformer.` prefix.  The reference picks the prefix by model name; here the file decides, by which of
// `wte.weight` / `transformer.wte.weight` it holds.  The causal-mask buffers older files carry (h.N.attn.bias,
// h.N.attn.masked_bias) and a stored lm_head.weight are never read: the head is wte.  The Conv1D matrices are stored
// [in, out] and are transposed once, here on the host, into the [out, in] rows the kernels read.
void LlmModel::load_gpt2(SafeTensors& st, int weights)
{
    gpt2_ = true;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, I = c.inter;
    std::string p;
    if (st.contains("wte.weight")) p = "";
    else if (st.contains("transformer.wte.weight")) p = "transformer.";
    else throw std::runtime_error("GPT-2 checkpoint without wte.weight or transformer.wte.weight");
    bf16_ = weights == 2 || (weights == 0 && st.get(p + "wte.weight").dtype == "BF16");
    std::vector<float> buf, t;
    auto read = [&](const std::string& name, std::vector<int64_t> want) {
        if (!st.contains(name)) throw std::runtime_error("missing tensor " + name);
        if (st.read_f32(name, buf) != want) throw std::runtime_error("tensor " + name + " has an unexpected shape");
    };
    auto vec = [&](const std::string& name, int n) {
        read(name, {n});
        return upload_f32(buf);
    };
    auto conv1d = [&](const std::string& name, int in, int out) {  // Conv1D [in, out] -> [out, in]
        read(name, {in, out});
        t.resize(buf.size());
        for (int i = 0; i < in; ++i)
            for (int o = 0; o < out; ++o) t[(size_t)o * in + i] = buf[(size_t)i * out + o];
        return upload_weight(t);
    };
    layers_.resize((size_t)c.layers);
    for (int i = 0; i < c.layers; ++i) {
        const std::string q = p + "h." + std::to_string(i) + ".";
        Layer& L = layers_[(size_t)i];
        L.up = nullptr;
        const TensorView& fc = st.get(q + "mlp.c_fc.weight");  // the intermediate width: n_inner when set, else 4 x n_embd
        if (fc.shape.size() != 2 || fc.shape[0] != H || fc.shape[1] != I)
            throw std::runtime_error("tensor " + q + "mlp.c_fc.weight has an unexpected shape (want [" + std::to_string(H) + ", " +
                                     std::to_string(I) + "] from n_inner / 4 x n_embd)");
        L.ln1 = vec(q + "ln_1.weight", H);
        L.ln1_b = vec(q + "ln_1.bias", H);
        L.wqkv = conv1d(q + "attn.c_attn.weight", H, 3 * H);
        L.bqkv = vec(q + "attn.c_attn.bias", 3 * H);
        L.wo = conv1d(q + "attn.c_proj.weight", H, H);
        L.bo = vec(q + "attn.c_proj.bias", H);
        L.ln2 = vec(q + "ln_2.weight", H);
        L.ln2_b = vec(q + "ln_2.bias", H);
        L.gate = conv1d(q + "mlp.c_fc.weight", H, I);
        L.bfc = vec(q + "mlp.c_fc.bias", I);
        L.down = conv1d(q + "mlp.c_proj.weight", I, H);
        L.bdown = vec(q + "mlp.c_proj.bias", H);
        L.k_cache = dalloc((size_t)cache_cap_ * H);
        L.v_cache = dalloc((size_t)cache_cap_ * H);
    }
    read(p + "wte.weight", {c.vocab, H});
    embed_ = lm_head_ = upload_weight(buf);
    read(p + "wpe.weight", {c.max_pos, H});
    wpe_ = upload_weight(buf);
    final_norm_ = vec(p + "ln_f.weight", H);
    final_norm_b_ = vec(p + "ln_f.bias", H);
}

void LlmModel::reset()
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    cache_len_ = 0;
    resident_.clear();
    hip_check(hipMemsetAsync(pos_, 0, sizeof(int), stream_), "reset pos");
    hip_check(hipMemsetAsync(count_, 0, sizeof(int), stream_), "reset count");
}

// ---------------------------------------------------------------------------------------------------------------------
// Prefix reuse.  resident_[i] is the token behind cache row i; a call that starts a sequence keeps the rows of the longest
// common prefix of resident_ and its prompt, capped so that every row whose output the call needs is computed by the call.

size_t prefix_keep_host(const uint32_t* resident, size_t n_resident, const uint32_t* prompt, size_t n_prompt, size_t limit)
{
    const size_t top = std::min(std::min(n_resident, n_prompt), limit);
    size_t p = 0;
    while (p < top && resident[p] == prompt[p]) ++p;
    return p;
}

int LlmModel::keep_prefix(const uint32_t* prompt, size_t n, size_t limit)
{
    const size_t p = prefix_keep_host(resident_.data(), resident_.size(), prompt, n, limit);
    cache_len_ = (int)p;  // rows [p, ...) are dead: the forward below overwrites them from p on
    resident_.resize(p);
    prefix_reused_ += p;
    prefix_computed_ += n - p;
    hip_check(hipMemsetAsync(pos_, 0, sizeof(int), stream_), "reset pos");  // (as reset(): forward() sets it to the new length)
    hip_check(hipMemsetAsync(count_, 0, sizeof(int), stream_), "reset count");
    return (int)p;
}

void LlmModel::begin_sequence(const std::vector<uint32_t>& prompt)
{
    if (!prefix_reuse_) {
        reset();
        forward(prompt.data(), (int)prompt.size());
        return;
    }
    // the last prompt token is always forwarded: its logits decide the first new token
    const int p = keep_prefix(prompt.data(), prompt.size(), prompt.size() - 1);
    forward(prompt.data() + p, (int)prompt.size() - p);
}

// What a generate loop leaves: `all` = the prompt + the emitted tokens.  Every one of them that was fed sits in the row of its
// index; the last emitted token may not have been fed, and rows past `all` belong to tokens the loop computed and discarded
// (a burst past a stop, rejected draft rows), so they do not count.
void LlmModel::leave_resident(const std::vector<uint32_t>& all)
{
    resident_.assign(all.begin(), all.begin() + (ptrdiff_t)std::min(all.size(), (size_t)cache_len_));
}

void LlmModel::project(StepRoute route, const LlmGemvArgs& a, const char* what)
{
    if (route == StepRoute::Step) {
        hip_check(launch_llm_gemv(a, stream_), what);
        return;
    }
    int streamed = 0;
    hip_check(launch_llm_gemv_lanes(a, stream_, &streamed), what);
    if (route == StepRoute::Verify) ++(streamed ? verify_stream_calls_ : verify_fallback_calls_);
    else ++(streamed ? lane_stream_calls_ : lane_fallback_calls_);
}

void LlmModel::embed_rows(const uint32_t* ids, int n, float* dst, int pos, const int* pos_ptr, const int* row_pos)
{
    const LlmConfig& c = cfg_;
    const int wb = bf16_ ? 1 : 0;
    if (quant_ && !fp8_) hip_check(launch_qembed(ids, n, qembed_, dst, stream_), "embed");
    else if (gpt2_) hip_check(launch_llm_embed_pos(ids, n, c.hidden, c.vocab, embed_, wpe_, c.max_pos, wb, pos, pos_ptr, dst, stream_, row_pos), "embed");
    else hip_check(launch_llm_embed(ids, n, c.hidden, c.vocab, embed_, wb, dst, stream_), "embed");
}

void LlmModel::final_norm(const float* src, int rows, float* dst)
{
    if (gpt2_) hip_check(launch_layernorm(src, final_norm_, final_norm_b_, cfg_.eps, rows, cfg_.hidden, dst, stream_), "ln_f");
    else hip_check(launch_rmsnorm(src, final_norm_, cfg_.eps, rows, cfg_.hidden, dst, stream_), "final norm");
}

void LlmModel::qlinear(const QMat& W, const float* X, int64_t ldx, int rows, bool linear, float* Y, int64_t ldy, const char* what)
{
    QGemvArgs a;
    a.W = W; a.X = X; a.ldx = ldx; a.rows = rows; a.Y = Y; a.ldy = ldy;
    if (linear && W.type == GGML_Q6_K) {  // Q6_K x Q8_K (matmul.rs:820-875): the activation rows quantized first
        hip_check(launch_q8k_quantize(X, ldx, rows, W.k, xq_, xd_, nullptr, stream_), what);
        a.Xq = xq_;
        a.Xd = xd_;
    }
    hip_check(launch_qgemv(a, stream_), what);
}

namespace {

bool q6(const QMat& m) { return m.type == GGML_Q6_K; }

}  // namespace

void LlmModel::quant_source(QFusedArgs& a, int n, const float* X, int ldx, int k, const float* gamma, bool q8k, const char* what)
{
    a.k = k; a.rows = n;
    if (!q8k) {
        a.X = X; a.ldx = ldx; a.gamma = gamma; a.eps = cfg_.eps;
        return;
    }
    hip_check(launch_qprep(X, ldx, n, k, gamma, cfg_.eps, gamma ? xn_ : nullptr, xq_, xd_, stream_), what);
    a.X = gamma ? xn_ : X; a.ldx = gamma ? k : ldx; a.Xq = xq_; a.Xd = xd_;
}

void LlmModel::quant_finish(int n, const Layer& L)
{
    hipStream_t s = stream_;
    const int H = cfg_.hidden, I = cfg_.inter;
    QFusedArgs o;
    quant_source(o, n, ctx_, H, H, nullptr, q6(L.o), "q8k o");
    o.W[0] = L.o; o.seg_jobs[0] = o.jobs = H / 2; o.R = h_; o.ldr = H; o.Y[0] = h_; o.ldy[0] = H;
    hip_check(launch_qfused(o, s), "o proj");
    QFusedArgs g;
    g.mode = QF_SWIGLU;
    quant_source(g, n, h_, H, H, L.ln2, q6(L.gate_q) || q6(L.up_q), "norm + q8k 2");
    g.W[0] = L.gate_q; g.W[1] = L.up_q; g.jobs = I; g.Y[0] = mid_; g.ldy[0] = I;
    hip_check(launch_qfused(g, s), "norm + gate/up");
    QFusedArgs dn;
    quant_source(dn, n, mid_, I, I, nullptr, q6(L.down_q), "q8k down");
    dn.W[0] = L.down_q; dn.seg_jobs[0] = dn.jobs = H / 2; dn.R = h_; dn.ldr = H; dn.Y[0] = h_; dn.ldy[0] = H;
    hip_check(launch_qfused(dn, s), "down proj");
}

void LlmModel::fp8_qkv(int n, const Layer& L, float* q, int64_t ldq, float* kdst, float* vdst, int64_t ldkv, int row_off, const int* row_off_ptr)
{
    Fp8ProjArgs a;
    a.mode = F8_QKV;
    a.W[0] = L.fq; a.W[1] = L.fk; a.W[2] = L.fv;
    a.X = h_; a.ldx = cfg_.hidden; a.rows = n; a.gamma = L.ln1; a.eps = cfg_.eps; a.bias = L.bqkv;
    a.Y[0] = q; a.ldy[0] = ldq; a.Y[1] = kdst; a.Y[2] = vdst; a.ldy[1] = a.ldy[2] = ldkv;
    a.row_off = row_off; a.row_off_ptr = row_off_ptr;
    hip_check(launch_fp8_proj(a, stream_), "norm + qkv");
}

void LlmModel::fp8_finish(int n, const Layer& L)
{
    hipStream_t s = stream_;
    const int H = cfg_.hidden, I = cfg_.inter, QD = cfg_.q_dim();
    Fp8ProjArgs o;
    o.W[0] = L.fo; o.X = ctx_; o.ldx = QD; o.rows = n; o.R = h_; o.ldr = H; o.Y[0] = h_; o.ldy[0] = H;
    hip_check(launch_fp8_proj(o, s), "o proj");
    Fp8ProjArgs g;
    g.mode = F8_SWIGLU;
    g.W[0] = L.fgate; g.W[1] = L.fup; g.X = h_; g.ldx = H; g.rows = n; g.gamma = L.ln2; g.eps = cfg_.eps; g.Y[0] = mid_; g.ldy[0] = I;
    hip_check(launch_fp8_proj(g, s), "norm + gate/up");
    Fp8ProjArgs dn;
    dn.W[0] = L.fdown; dn.X = mid_; dn.ldx = I; dn.rows = n; dn.R = h_; dn.ldr = H; dn.Y[0] = h_; dn.ldy[0] = H;
    hip_check(launch_fp8_proj(dn, s), "down proj");
}

void LlmModel::head(StepRoute route, const float* X, int rows, float* Y, bool norm_in_head)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden;
    if (quant_ && !fp8_) {  // (the quantized kernels take <= 8 rows as they are; an FP8 checkpoint's head is f32 / bf16)
        qlinear(qhead_, X, H, rows, head_q8k_, Y, c.vocab, "lm head");
        return;
    }
    LlmGemvArgs lm;
    lm.X = X; lm.ldx = H; lm.rows = rows; lm.W = lm_head_; lm.bf16 = bf16_; lm.n_out = c.vocab; lm.k = H; lm.Y0 = Y; lm.ldy0 = c.vocab;
    if (norm_in_head) {
        lm.gamma = final_norm_; lm.eps = c.eps; lm.norm_out = last_;
    }
    project(route, lm, "lm head");
}

// Norm + Q | K | V + rotation of n rows (decoder_attention.rs:61-82), three forms.  Quantized matrices: one fused launch
// (quant_kernels.hip: RMSNorm + per-segment types + RoPE + cache write; a Q6_K linear first takes one qprep launch,
// quant_source()).  fused: the one-token Llama launch.  Else the GEMV with the K / V segments landing in the cache rows, then
// the rotation where they sit: Qwen3 head norm + RoPE in one launch, Llama RoPE of Q and of K, GPT-2 (learned positions) none.
// FP8 matrices take that last form with fp8_qkv() (fp8_kernels.hip) as the GEMV.
void LlmModel::step_qkv(StepRoute route, int n, const Layer& L, const int* pos, bool fused, const uint32_t* embed_ids)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, d = c.head_dim, kv = c.kv_heads * d, QD = c.q_dim();
    if (fp8_) {  // plain segments (Q of q_dim() columns, K / V into the cache rows), then the rotation where they sit
        fp8_qkv(n, L, q_, QD, L.k_cache, L.v_cache, kv, cache_len_, pos);
        if (c.qwen3()) {
            hip_check(launch_qk_norm_rope(q_, QD, L.k_cache, kv, n, c.heads, c.kv_heads, d, L.q_norm, L.k_norm, c.eps, cos_, sin_, cache_len_, pos, 1,
                                          s), "qk norm + rope");
        } else {
            hip_check(launch_rope(q_, QD, n, c.heads, d, cos_, sin_, cache_len_, pos, 0, s), "rope q");
            hip_check(launch_rope(L.k_cache, kv, n, c.kv_heads, d, cos_, sin_, cache_len_, pos, 1, s), "rope k");
        }
        return;
    }
    if (quant_) {
        QFusedArgs qkv;
        qkv.mode = QF_QKV;
        quant_source(qkv, n, h_, H, H, L.ln1, q6(L.q) || q6(L.k) || q6(L.v), "norm + q8k 1");
        qkv.W[0] = L.q; qkv.W[1] = L.k; qkv.W[2] = L.v;
        qkv.seg_jobs[0] = H / 2; qkv.seg_jobs[1] = kv / 2; qkv.seg_jobs[2] = kv / 2;
        qkv.jobs = H / 2 + kv;
        qkv.bias = L.bqkv; qkv.bias_off[1] = H; qkv.bias_off[2] = H + kv;
        qkv.Y[0] = q_; qkv.ldy[0] = H; qkv.Y[1] = L.k_cache; qkv.Y[2] = L.v_cache; qkv.ldy[1] = qkv.ldy[2] = kv;
        qkv.row_off = cache_len_; qkv.row_off_ptr = pos;
        qkv.head_dim = d; qkv.cos_t = cos_; qkv.sin_t = sin_;
        hip_check(launch_qfused(qkv, s), "norm + qkv + rope");
        return;
    }
    if (fused) {
        hip_check(launch_llm_qkv_rope(h_, L.ln1, c.eps, L.wqkv, bf16_ ? 1 : 0, L.bqkv, H, c.heads, c.kv_heads, d, cos_, sin_, q_, L.k_cache,
                                      L.v_cache, cache_len_, pos, s, embed_ids, embed_ids ? embed_ : nullptr, c.vocab, embed_ids ? h_ : nullptr),
                  "norm + qkv + rope");
        return;
    }
    LlmGemvArgs a;
    a.X = h_; a.ldx = H; a.rows = n; a.gamma = L.ln1; a.beta = L.ln1_b; a.layernorm = gpt2_ ? 1 : 0; a.eps = c.eps; a.W = L.wqkv;
    a.bf16 = bf16_; a.bias = L.bqkv; a.n_out = QD + 2 * kv; a.k = H; a.seg_q = QD; a.seg_kv = kv; a.Y0 = q_; a.ldy0 = QD;
    a.Y1 = L.k_cache; a.Y2 = L.v_cache; a.ldy12 = kv; a.row_off = cache_len_; a.row_off_ptr = pos;
    project(route, a, "norm + qkv");
    if (c.qwen3()) {
        hip_check(launch_qk_norm_rope(q_, QD, L.k_cache, kv, n, c.heads, c.kv_heads, d, L.q_norm, L.k_norm, c.eps, cos_, sin_, cache_len_, pos, 1,
                                      s), "qk norm + rope");
    } else if (!gpt2_) {
        hip_check(launch_rope(q_, QD, n, c.heads, d, cos_, sin_, cache_len_, pos, 0, s), "rope q");
        hip_check(launch_rope(L.k_cache, kv, n, c.kv_heads, d, cos_, sin_, cache_len_, pos, 1, s), "rope k");
    }
}

void LlmModel::layer_finish(StepRoute route, int n, const Layer& L, bool slabs)
{
    if (quant_) {
        if (fp8_) fp8_finish(n, L);
        else quant_finish(n, L);
        return;
    }
    const LlmConfig& c = cfg_;
    const int H = c.hidden, I = c.inter, QD = c.q_dim();
    LlmGemvArgs o;
    o.X = ctx_; o.ldx = QD; o.rows = n; o.W = L.wo; o.bf16 = bf16_; o.bias = L.bo; o.R = h_; o.ldr = H; o.n_out = H; o.k = QD; o.Y0 = h_; o.ldy0 = H;
    if (slabs) {
        o.X = att_scratch_; o.att_splits = splits_; o.att_head_dim = c.head_dim;
    }
    project(route, o, "o proj");
    if (L.moe) {
        moe_steps(n, L);
        return;
    }
    LlmGemvArgs g;  // RMSNorm + SwiGLU (swiglu.rs:32-57); GPT-2: LayerNorm(ln_2) + c_fc + bias + GELU-tanh
    g.X = h_; g.ldx = H; g.rows = n; g.gamma = L.ln2; g.beta = L.ln2_b; g.eps = c.eps; g.W = L.gate; g.bf16 = bf16_; g.bias = L.bfc;
    g.n_out = I; g.k = H; g.Y0 = mid_; g.ldy0 = I;
    if (gpt2_) {
        g.layernorm = 1; g.gelu_tanh = 1;
    } else {
        g.W2 = L.up; g.swiglu = 1;
    }
    project(route, g, "norm + mlp in");
    LlmGemvArgs dn;
    dn.X = mid_; dn.ldx = I; dn.rows = n; dn.W = L.down; dn.bf16 = bf16_; dn.bias = L.bdown; dn.R = h_; dn.ldr = H; dn.n_out = H; dn.k = I;
    dn.Y0 = h_; dn.ldy0 = H;
    project(route, dn, "down proj");
}

// The sparse FFN of a qwen3_moe layer behind the o-proj (moe_kernels.h), in place on the residual stream.  The routing record of
// the layer is what the route kernel writes: the last pass's ids and weights stay readable (moe_routing()).
namespace {

MoeFfnArgs moe_args(const LlmConfig& c, bool bf16)
{
    MoeFfnArgs a;
    a.E = c.num_experts; a.k = c.experts_per_tok; a.Im = c.moe_inter; a.H = c.hidden; a.norm_topk = c.norm_topk ? 1 : 0; a.eps = c.eps;
    a.bf16 = bf16 ? 1 : 0;
    return a;
}

}  // namespace

void LlmModel::moe_steps(int n, const Layer& L)
{
    const int H = cfg_.hidden;
    MoeFfnArgs a = moe_args(cfg_, bf16_);
    a.X = h_; a.ldx = H; a.rows = n; a.gamma = L.ln2;
    a.router = L.router; a.gate = L.gate_stack; a.up = L.up_stack; a.down = L.down_stack;
    a.R = h_; a.ldr = H; a.Y = h_; a.ldy = H;
    a.logits = moe_logits_; a.ids = L.moe_ids; a.weights = L.moe_weights; a.mid = moe_mid_;
    hip_check(launch_moe_ffn_steps(a, stream_), "moe ffn (steps)");
    L.moe_rec_rows = n;
}

void LlmModel::moe_rows(int m, const Layer& L)
{
    const int H = cfg_.hidden, k = cfg_.experts_per_tok;
    if (m > kMoeRecordRows) throw std::runtime_error("moe_rows: more rows than the routing record holds");
    for (int r0 = 0; r0 < m; r0 += kMoeBlockRows) {
        const int rows = std::min(kMoeBlockRows, m - r0);
        MoeFfnArgs a = moe_args(cfg_, bf16_);
        float* h = ph_ + (size_t)r0 * H;
        a.X = h; a.ldx = H; a.rows = rows; a.gamma = L.ln2; a.xn = pn_ + (size_t)r0 * H;
        a.router = L.router; a.gate = L.gate_stack; a.up = L.up_stack; a.down = L.down_stack;
        a.R = h; a.ldr = H; a.Y = h; a.ldy = H;
        a.logits = pmoe_logits_; a.ids = L.moe_ids + (size_t)r0 * k; a.weights = L.moe_weights + (size_t)r0 * k;
        a.mid = pmoe_mid_; a.y = pmoe_y_; a.plan = pmoe_plan_;
        hip_check(launch_moe_ffn_grouped(a, stream_), "moe ffn (rows)");
    }
    L.moe_rec_rows = m;
}

int LlmModel::moe_record_rows(int layer) const
{
    if (!cfg_.moe()) throw InvalidConfig("moe_routing: the model is dense (model_type '" + cfg_.model_type + "')");
    if (layer < 0 || layer >= cfg_.layers) throw InvalidConfig("moe_routing: layer must be 0 .. " + std::to_string(cfg_.layers - 1));
    if (!layers_[(size_t)layer].moe) throw InvalidConfig("moe_routing: layer " + std::to_string(layer) + " is a dense layer");
    return layers_[(size_t)layer].moe_rec_rows;
}

void LlmModel::moe_routing(int layer, int32_t* ids_out, float* weights_out)
{
    const int rows = moe_record_rows(layer);
    if (rows <= 0) return;
    const Layer& L = layers_[(size_t)layer];
    const size_t n = (size_t)rows * cfg_.experts_per_tok;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    hip_check(hipMemcpy(ids_out, L.moe_ids, n * 4, hipMemcpyDeviceToHost), "D2H moe ids");
    hip_check(hipMemcpy(weights_out, L.moe_weights, n * 4, hipMemcpyDeviceToHost), "D2H moe weights");
}

// One pass of n <= 8 rows for every family (llama/cpu_decoder.rs:142-219, gpt2/cpu_decoder.rs:371-394): the embedding (GPT-2:
// token + learned position), per layer step_qkv -> attention -> layer_finish, then the final norm and the vocabulary head.
// The one-token step (n == 1, not verify) fuses where the kernels allow: the Llama layer's norm + Q|K|V + RoPE in one launch,
// whose first layer also gathers the embedding row; the attention's slab merge inside the output projection (not quantized);
// the final norm inside the head (Llama / Qwen3).
void LlmModel::pass(const uint32_t* ids_dev, int n, bool device_pos, bool verify)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden, d = c.head_dim, kv = c.kv_heads * d, QD = c.q_dim();
    const StepRoute route = verify ? StepRoute::Verify : StepRoute::Step;
    const int* pp = device_pos ? pos_ : nullptr;
    const bool one = n == 1 && !verify, llama = !quant_ && !gpt2_;
    const bool fused_qkv = one && llama && !c.qwen3() && H <= 8192;  // (Qwen3 normalises Q and K per head between projection and rotation)
    const bool embed_in_qkv = fused_qkv && !layers_.empty() && llm_qkv_rope_embeds(H, layers_[0].ln1, layers_[0].wqkv, embed_);
    const bool merge_in_proj = one && !quant_ && llm_gemv_merges_attention(QD, splits_, d);  // no combine launch
    if (!embed_in_qkv) embed_rows(ids_dev, n, h_, cache_len_, pp, nullptr);
    for (const Layer& L : layers_) {
        step_qkv(route, n, L, pp, fused_qkv, embed_in_qkv && &L == &layers_[0] ? ids_dev : nullptr);
        hip_check(launch_decode_attention(q_, QD, n, L.k_cache, kv, L.v_cache, kv, cache_len_ + n, pp, cache_cap_, c.heads, d, cache_len_,
                                          splits_, att_scratch_, merge_in_proj ? nullptr : ctx_, QD, stream_, c.heads / c.kv_heads), "attention");
        layer_finish(route, n, L, merge_in_proj);
    }
    if (one && (llama || fp8_) && llm_gemv_streams(H, lm_head_, nullptr)) {  // the head normalises the row itself (and stores it in last_)
        head(route, h_, 1, logits_, true);
        return;
    }
    final_norm(h_, n, last_);  // every row: forward_rows() scores from them
    if (verify) head(route, last_, n, vlogits_);  // every row's logits
    else head(route, last_ + (size_t)(n - 1) * H, 1, logits_);
}

void LlmModel::ensure_prompt_workspace()
{
    if (ph_) return;
    const int H = cfg_.hidden, kv = cfg_.kv_heads * cfg_.head_dim, I = cfg_.inter, QD = cfg_.q_dim();
    prefill_cap_ = 2048;
    const size_t P = (size_t)prefill_cap_;
    ph_ = dalloc(P * H);
    pn_ = dalloc(P * H);
    pq_ = dalloc(P * QD);
    pctx_ = dalloc(P * QD);
    pg_ = dalloc(P * I);
    pu_ = dalloc(P * I);
    pids_ = reinterpret_cast<uint32_t*>(dalloc(P));
    psplit_ = dalloc(prefill_gemm_scratch_floats(prefill_cap_, std::max(I, std::max(H, QD))));
    if (bf16_ || quant_) pw32_ = dalloc(std::max((size_t)(QD + 2 * kv) * H, (size_t)I * H));
    if (quant_) pact_ = dalloc(P * (size_t)std::max(H, I));
    if (cfg_.moe()) {  // the slot-major scratch of one block of rows: kMoeBlockRows * k * (hidden + Im) floats
        const size_t B = (size_t)kMoeBlockRows, k = (size_t)cfg_.experts_per_tok;
        pmoe_logits_ = dalloc(B * cfg_.num_experts);
        pmoe_mid_ = dalloc(B * k * cfg_.moe_inter);
        pmoe_y_ = dalloc(B * k * H);
        pmoe_plan_ = reinterpret_cast<int32_t*>(dalloc(moe_plan_ints((int)(B * k), cfg_.num_experts)));
    }
}

// Y[m, N] = A W^T (+ bias) (+ R), or with `gate`: gate = silu(gate) * (A W^T).  Blocks of >= kTileRows rows run the
// encoder's 128 x 128-tile f32 GEMM (gemm.hip), bf16 weights on an f32 copy made just before (100 MB moved per 69 GFLOP
// at 2 048 rows).  Measured on the 1B shape: 2 048 rows 46.2 -> 42.6 ms, 1 792 rows 40.4 -> 39.1 ms, 1 536 rows 33.1 -> 36.1 ms
// (the 2 048-wide projections are then 192 tiles on 256 CUs): hence kTileRows.
// per projection: the 128 x 128 tiles when they number at least one per CU (m / 128 x N / 128 >= 208), from kTileRows rows
// gelu (GPT-2's c_fc): Y = gelu_tanh(A W^T + bias), in the f32 tile GEMM's epilogue, else as a pass over Y after the GEMM
void LlmModel::prompt_proj(int m, const float* Ain, int lda, const void* W, const float* bias, const float* R, float* Y, int ldy, int N, int K,
                           float* gate, const char* what, const QMat* qm, bool gelu, const Fp8Mat* fm)
{
    hipStream_t s = stream_;
    const int H = cfg_.hidden, kv = cfg_.kv_heads * cfg_.head_dim, I = cfg_.inter, QD = cfg_.q_dim();
    constexpr int kTileRows = 512;  // rows from which a projection may take the encoder's 128 x 128-tile f32 GEMM (if its tiles fill the chip)
    const bool tile_shapes = H % 128 == 0 && QD % 128 == 0 && I % 128 == 0 && kv % 128 == 0 && (!bf16_ || pw32_);
    // a quantized matrix: dequantized into the f32 scratch first; a Q6_K linear also takes its activation rows through
    // Q8_K and back (the quantization the decode kernels apply), then everything is the f32 route
    int wbu = bf16_ ? 1 : 0;
    bool bf = bf16_;
    // measured on the 1B shape: 192 tiles (1 536 rows x 2 048 columns) are faster on the 64 x 64 kernel, 224 on the tiles -- with
    // f32 weights (both kernels on the f32 matrix cores) and again with bf16 weights (both on the bf16 matrix cores: 768 /
    // 1 024 tokens 8.1 / 9.8 ms at 208 against 9.9 / 11.2 at 96 and 8.8 / 11.2 with no tiles at all)
    constexpr int min_tiles = 208;
    const bool tiles = tile_shapes && m >= kTileRows && (int64_t)((m + 127) / 128) * (N / 128) >= min_tiles;
    if (fm && fp8_mc_ && !tiles) {  // the switch: the codes themselves on the bf16 matrix cores, no f32 copy of the matrix
        hip_check(launch_prefill_gemm_fp8(Ain, lda, *fm, bias, R, ldy, Y, ldy, m, s, psplit_, gate), what);
        return;
    }
    if (fm) {  // an FP8 matrix: decode(code) * scale into the f32 scratch, then the f32 route
        hip_check(launch_fp8_dequant(*fm, pw32_, s), what);
        W = pw32_;
        wbu = 0;
        bf = false;
    } else if (qm) {
        hip_check(launch_qdequant(*qm, pw32_, s), what);
        if (qm->type == GGML_Q6_K) {
            hip_check(launch_q8k_quantize(Ain, lda, m, K, nullptr, nullptr, pact_, s), what);
            Ain = pact_;
            lda = K;
        }
        W = pw32_;
        wbu = 0;
        bf = false;
    }
    if (!tiles) {
        hip_check(launch_prefill_gemm(Ain, lda, W, wbu, bias, R, ldy, Y, ldy, m, N, K, s, psplit_, gate), what);
        if (gelu) hip_check(launch_gelu_tanh(Y, (size_t)m * N, s), what);
        return;
    }
    ++tile_gemm_calls_;
    // bf16 weights: the bf16 matrix cores take them as they are, the f32 activations as three exact bf16 pieces (the same
    // products as the f32 GEMM on a widened copy: gemm_split.hip) -- 2 048-token prompt 33.8 -> 18.1 ms, no 100 MB copy
    if (bf && K % 64 == 0) {
        if (gate)
            hip_check(launch_gemm_bf16_weights(Ain, lda, W, bias, gate, ldy, gate, ldy, m, N, K, EPI_BIAS_MUL_SILU, s), what);
        else
            hip_check(launch_gemm_bf16_weights(Ain, lda, W, bias, R, ldy, Y, ldy, m, N, K, R ? EPI_BIAS_RESIDUAL : EPI_BIAS, s), what);
        if (gelu) hip_check(launch_gelu_tanh(Y, (size_t)m * N, s), what);
        return;
    }
    const float* W32 = static_cast<const float*>(W);
    if (bf) {
        hip_check(launch_widen_bf16(W, pw32_, (size_t)N * K, s), "widen");
        W32 = pw32_;
    }
    if (gate)
        hip_check(launch_gemm(Ain, lda, W32, bias, gate, ldy, gate, ldy, m, N, K, EPI_BIAS_MUL_SILU, s), what);
    else
        hip_check(launch_gemm(Ain, lda, W32, bias, R, ldy, Y, ldy, m, N, K, gelu ? EPI_BIAS_GELU_NEW : (R ? EPI_BIAS_RESIDUAL : EPI_BIAS), s),
                  what);
}

// The first half of a rows-route layer: RMSNorm (GPT-2: LayerNorm) of ph_ into pn_, then the Q, K and V projections out of the
// fused Q|K|V matrix (quantized checkpoints: three matrices of their own), Q into pq_, K and V into the rows given.
void LlmModel::rows_qkv(int m, const Layer& L, float* k_rows, float* v_rows)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, kv = c.kv_heads * c.head_dim, QD = c.q_dim();
    const size_t wsz = bf16_ ? 2 : 4;
    auto at = [&](const void* w, size_t elems) { return static_cast<const void*>(static_cast<const char*>(w) + elems * wsz); };
    auto gq = [&](const QMat& m) { return quant_ && !fp8_ ? &m : nullptr; };  // the layer's matrix as prompt_proj's qm / fm
    auto fq = [&](const Fp8Mat& m) { return fp8_ ? &m : nullptr; };
    if (gpt2_) hip_check(launch_layernorm(ph_, L.ln1, L.ln1_b, c.eps, m, H, pn_, s), "ln_1");
    else hip_check(launch_rmsnorm(ph_, L.ln1, c.eps, m, H, pn_, s), "rmsnorm 1");
    prompt_proj(m, pn_, H, L.wqkv, L.bqkv, nullptr, pq_, QD, QD, H, nullptr, "q proj", gq(L.q), false, fq(L.fq));
    prompt_proj(m, pn_, H, quant_ ? nullptr : at(L.wqkv, (size_t)QD * H), L.bqkv ? L.bqkv + QD : nullptr, nullptr, k_rows, kv, kv, H, nullptr,
                "k proj", gq(L.k), false, fq(L.fk));
    prompt_proj(m, pn_, H, quant_ ? nullptr : at(L.wqkv, (size_t)(QD + kv) * H), L.bqkv ? L.bqkv + QD + kv : nullptr, nullptr, v_rows, kv, kv, H,
                nullptr, "v proj", gq(L.v), false, fq(L.fv));
}

// The second half, behind the attention's context rows in pctx_: o-proj + residual -> RMSNorm -> gate, up -> silu(gate) * up ->
// down-proj + residual (GPT-2: LayerNorm -> c_fc + GELU -> mlp.c_proj + residual), the hidden states staying in ph_.
void LlmModel::rows_finish(int m, const Layer& L)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, I = c.inter, QD = c.q_dim();
    auto gq = [&](const QMat& m) { return quant_ && !fp8_ ? &m : nullptr; };
    auto fq = [&](const Fp8Mat& m) { return fp8_ ? &m : nullptr; };
    prompt_proj(m, pctx_, QD, L.wo, L.bo, ph_, ph_, H, H, QD, nullptr, "o proj", gq(L.o), false, fq(L.fo));
    if (gpt2_) {
        hip_check(launch_layernorm(ph_, L.ln2, L.ln2_b, c.eps, m, H, pn_, s), "ln_2");
        prompt_proj(m, pn_, H, L.gate, L.bfc, nullptr, pg_, I, I, H, nullptr, "c_fc", nullptr, true);
        prompt_proj(m, pg_, I, L.down, L.bdown, ph_, ph_, H, H, I, nullptr, "mlp c_proj");
        return;
    }
    if (L.moe) {
        moe_rows(m, L);
        return;
    }
    hip_check(launch_rmsnorm(ph_, L.ln2, c.eps, m, H, pn_, s), "rmsnorm 2");
    prompt_proj(m, pn_, H, L.gate, nullptr, nullptr, pg_, I, I, H, nullptr, "gate", gq(L.gate_q), false, fq(L.fgate));
    prompt_proj(m, pn_, H, L.up, nullptr, nullptr, pu_, I, I, H, pg_, "up + swiglu", gq(L.up_q), false, fq(L.fup));
    prompt_proj(m, pg_, I, L.down, nullptr, ph_, ph_, H, H, I, nullptr, "down proj", gq(L.down_q), false, fq(L.fdown));
}

// Prompt rows through the fp32 matrix cores (prefill_gemm_kernel) instead of 8-row GEMV passes: per layer rows_qkv() (K and V
// rows land in the cache) -> RoPE -> causal attention over the cache -> rows_finish(); same formulas as pass().  After the last
// layer the final norm runs on the last (n - 1) % 8 + 1 rows (what last_hidden() exposes) and the lm head on the last row.
void LlmModel::prefill_rows(const uint32_t* ids_host, int n, bool score, int score_base)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, d = c.head_dim, kv = c.kv_heads * d, QD = c.q_dim();
    ensure_prompt_workspace();
    for (int done = 0; done < n; done += prefill_cap_) {
        const int m = std::min(prefill_cap_, n - done);
        hip_check(hipMemcpyAsync(pids_, ids_host + done, (size_t)m * 4, hipMemcpyHostToDevice, s), "H2D ids");
        embed_rows(pids_, m, ph_, cache_len_, nullptr, nullptr);
        for (const Layer& L : layers_) {
            rows_qkv(m, L, L.k_cache + (size_t)cache_len_ * kv, L.v_cache + (size_t)cache_len_ * kv);
            if (c.qwen3()) {  // head norm + rotation over the chunk's Q rows and its K rows in the cache
                hip_check(launch_qk_norm_rope(pq_, QD, L.k_cache, kv, m, c.heads, c.kv_heads, d, L.q_norm, L.k_norm, c.eps, cos_, sin_, cache_len_,
                                              nullptr, 1, s), "qk norm + rope");
            } else if (!gpt2_) {  // (GPT-2: learned positions, already in the embedding)
                hip_check(launch_rope(pq_, QD, m, c.heads, d, cos_, sin_, cache_len_, nullptr, 0, s), "rope q");
                hip_check(launch_rope(L.k_cache, kv, m, c.kv_heads, d, cos_, sin_, cache_len_, nullptr, 1, s), "rope k");
            }
            if (prefill_attention_supported(d)) {
                hip_check(launch_prefill_attention(pq_, QD, m, L.k_cache, kv, L.v_cache, kv, cache_len_, c.heads, d, c.heads / c.kv_heads, pctx_, QD, s),
                          "attention");
            } else {
                for (int r = 0; r < m; r += 8) {  // 8 query rows at a time against everything cached up to them
                    const int rows = std::min(8, m - r);
                    hip_check(launch_decode_attention(pq_ + (size_t)r * QD, QD, rows, L.k_cache, kv, L.v_cache, kv, cache_len_ + r + rows, nullptr,
                                                      cache_cap_, c.heads, d, cache_len_ + r, splits_, att_scratch_, pctx_ + (size_t)r * QD, QD, s,
                                                      c.heads / c.kv_heads), "attention");
                }
            }
            rows_finish(m, L);
        }
        if (score) {  // the chunk's rows whose successor is scored: final norm into the (now free) norm buffer, then the head
            const int at = score_base + done;  // the chunk's first position in the scored sequence
            const int lo = std::max(at, score_first_ - 1), hi = std::min(at + m - 1, score_n_ - 2);
            if (lo <= hi) {
                final_norm(ph_ + (size_t)(lo - at) * H, hi - lo + 1, pn_);
                score_head_rows(pn_, lo, hi - lo + 1);
            }
        }
        cache_len_ += m;
        if (done + m == n) {
            const int rows = (n - 1) % 8 + 1;
            final_norm(ph_ + (size_t)(m - rows) * H, rows, last_);
            head(StepRoute::Step, last_ + (size_t)(rows - 1) * H, 1, logits_);
            last_rows_ = rows;
        }
        hip_check(hipStreamSynchronize(s), "sync");  // pids_ and the activations are reused by the next chunk
    }
}

namespace {

// The two geometry rules of the rows route.  forward() takes it for widths the prompt GEMM tiles and any even head_dim (other
// shapes run pass() 8 rows at a time); the packed entry points have no such fallback, and their attention kernels exist for
// four head dims.
bool rows_geometry(const LlmConfig& c)
{
    return c.hidden % 32 == 0 && c.q_dim() % 32 == 0 && c.inter % 32 == 0 && (c.kv_heads * c.head_dim) % 4 == 0 && c.head_dim % 2 == 0;
}
bool packed_geometry(const LlmConfig& c)
{
    const int d = c.head_dim;
    return c.hidden % 32 == 0 && c.q_dim() % 32 == 0 && c.inter % 32 == 0 && (c.kv_heads * d) % 4 == 0 &&
           (d == 16 || d == 32 || d == 64 || d == 128);
}
std::string packed_geometry_refusal(const char* entry)
{
    return std::string(entry) + ": hidden, heads * head_dim and intermediate_size must be multiples of 32 and head_dim one of 16, 32, 64, 128";
}

}  // namespace

void LlmModel::forward(const uint32_t* ids, int n) { forward_rows(ids, n, false); }

void LlmModel::forward_rows(const uint32_t* ids, int n, bool score, int score_base)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (n < 1) throw std::runtime_error("forward needs at least one token");
    if (cache_len_ + n > cache_cap_) throw std::runtime_error("context is full");
    const bool tracked = resident_.size() == (size_t)cache_len_;  // (else: untracked rows lie between; resident_ stays a prefix)
    constexpr int kMinGemmRows = 24;  // rows from which the matrix-core route is used
    if (n >= kMinGemmRows && rows_geometry(cfg_)) {
        prefill_rows(ids, n, score, score_base);
    } else {
        for (int i = 0; i < n; i += 8) {
            const int m = std::min(8, n - i);
            hip_check(hipMemcpyAsync(ids_, ids + i, (size_t)m * 4, hipMemcpyHostToDevice, stream_), "H2D ids");
            pass(ids_, m, false);
            if (score) {  // pass() final-norms every row of the block into last_
                const int at = score_base + i;  // the block's first position in the scored sequence
                const int lo = std::max(at, score_first_ - 1), hi = std::min(at + m - 1, score_n_ - 2);
                if (lo <= hi) score_head_rows(last_ + (size_t)(lo - at) * cfg_.hidden, lo, hi - lo + 1);
            }
            cache_len_ += m;
            last_rows_ = m;
            hip_check(hipStreamSynchronize(stream_), "sync");  // ids_ is reused by the next block
        }
    }
    hip_check(hipMemcpyAsync(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    hip_check(hipStreamSynchronize(stream_), "sync");
    if (tracked) resident_.insert(resident_.end(), ids, ids + n);
}

void LlmModel::ensure_score()
{
    if (score_tgt_) return;
    const size_t cap = (size_t)cache_cap_;
    score_tgt_ = reinterpret_cast<uint32_t*>(dalloc(cap));
    score_top_ = reinterpret_cast<uint32_t*>(dalloc(cap));
    score_lp_ = dalloc(cap);
    score_tlp_ = dalloc(cap);
    for (int m = 64; m <= 2048; m += 64)  // a head launch has at most a prompt chunk's rows
        score_scratch_bytes_ = std::max(score_scratch_bytes_, score_head_scratch_bytes(m, cfg_.vocab, 0));
    score_scratch_ = dalloc((score_scratch_bytes_ + 3) / 4);
}

void LlmModel::ensure_score_topk()
{
    if (score_tk_ids_) return;
    const size_t cap = (size_t)cache_cap_ * KJARNI_SCORE_TOPK_MAX;
    score_tk_ids_ = reinterpret_cast<uint32_t*>(dalloc(cap));
    score_tk_lp_ = dalloc(cap);
    for (int m = 64; m <= 2048; m += 64)
        score_tk_scratch_bytes_ = std::max(score_tk_scratch_bytes_, score_head_topk_scratch_bytes(m, cfg_.vocab, 0, KJARNI_SCORE_TOPK_MAX));
    score_tk_scratch_ = dalloc((score_tk_scratch_bytes_ + 3) / 4);
}

void LlmModel::score_head_rows(const float* Xn, int lo, int cnt)
{
    const int out = lo + 1 - score_first_;
    const size_t kout = (size_t)out * score_k_;  // the rows' first slot in the top-k outputs
    if (score_k_ > 0) score_head(Xn, cnt, score_tgt_ + lo, score_k_, score_lp_ + out, score_tk_ids_ + kout, score_tk_lp_ + kout);
    else score_head(Xn, cnt, score_tgt_ + lo, 0, score_lp_ + out, score_top_ + out, score_tlp_ + out);
}

void LlmModel::score_head(const float* Xn, int cnt, const uint32_t* tgt, int k, float* lp, uint32_t* ids, float* tlp)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden;
    if (score_fused_ && (!quant_ || fp8_) && llm_score_head_takes(Xn, H, lm_head_, bf16_ ? 1 : 0, H)) {
        if (k > 0) {
            if (score_head_topk_scratch_bytes(cnt, c.vocab, 0, k) > score_tk_scratch_bytes_)
                throw std::runtime_error("score head: top-k slab scratch too small");
            hip_check(launch_score_head_topk(Xn, H, cnt, lm_head_, bf16_ ? 1 : 0, c.vocab, H, tgt, 0, k, score_tk_scratch_, lp, ids, tlp, nullptr,
                                             stream_), "score head top-k");
        } else {
            if (score_head_scratch_bytes(cnt, c.vocab, 0) > score_scratch_bytes_) throw std::runtime_error("score head: slab scratch too small");
            hip_check(launch_score_head(Xn, H, cnt, lm_head_, bf16_ ? 1 : 0, c.vocab, H, tgt, 0, score_scratch_, lp, ids, tlp, nullptr, stream_),
                      "score head");
        }
        ++score_fused_calls_;
        return;
    }
    ensure_lookup();  // vlogits_: the verify step's 8 logits rows
    const size_t slots = k > 0 ? (size_t)k : 1;  // per row in ids / tlp
    for (int r = 0; r < cnt; r += 8) {
        const int rows = std::min(8, cnt - r);
        head(StepRoute::Step, Xn + (size_t)r * H, rows, vlogits_);
        if (k > 0)
            hip_check(launch_score_rows_topk(vlogits_, c.vocab, rows, c.vocab, tgt + r, k, lp + r, ids + r * slots, tlp + r * slots, nullptr,
                                             stream_), "score rows top-k");
        else
            hip_check(launch_score_rows(vlogits_, c.vocab, rows, c.vocab, tgt + r, lp + r, ids + r * slots, tlp + r * slots, nullptr, stream_),
                      "score rows");
        ++score_rows_calls_;
    }
}

void LlmModel::score_pass(const uint32_t* ids, int n, int first, int top_k)
{
    if (n < 2) throw InvalidConfig("n (" + std::to_string(n) + ") must be at least 2: a scored token needs a prefix");
    if (first < 1 || first >= n) throw InvalidConfig("first (" + std::to_string(first) + ") must be in [1, n) with n = " + std::to_string(n));
    if (n > cache_cap_) throw InvalidConfig("n (" + std::to_string(n) + " tokens) exceeds the context of " + std::to_string(cache_cap_) + " tokens");
    for (int i = 0; i < n; ++i)
        if (ids[i] >= (uint32_t)cfg_.vocab)
            throw InvalidConfig("ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is not below the vocabulary size " +
                                std::to_string(cfg_.vocab));
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ensure_score();
    if (top_k > 0) ensure_score_topk();
    // prefix reuse: rows first - 1 .. n - 2 must reach the head, so at most first - 1 rows are kept; targets and result slots
    // stay indexed by absolute position
    int keep = 0;
    if (prefix_reuse_) keep = keep_prefix(ids, (size_t)n, (size_t)first - 1);
    else reset();
    hip_check(hipMemcpyAsync(score_tgt_, ids + 1, (size_t)(n - 1) * 4, hipMemcpyHostToDevice, stream_), "H2D targets");
    score_first_ = first;
    score_n_ = n;
    score_k_ = top_k;
    forward_rows(ids + keep, n - keep, true, keep);
}

void LlmModel::score(const uint32_t* ids, int n, int first, float* logprob_out, uint32_t* top_out, float* top_logprob_out)
{
    score_pass(ids, n, first, 0);
    const size_t cnt = (size_t)(n - first);
    if (logprob_out) hip_check(hipMemcpyAsync(logprob_out, score_lp_, cnt * 4, hipMemcpyDeviceToHost, stream_), "D2H logprob");
    if (top_out) hip_check(hipMemcpyAsync(top_out, score_top_, cnt * 4, hipMemcpyDeviceToHost, stream_), "D2H top");
    if (top_logprob_out) hip_check(hipMemcpyAsync(top_logprob_out, score_tlp_, cnt * 4, hipMemcpyDeviceToHost, stream_), "D2H top logprob");
    hip_check(hipStreamSynchronize(stream_), "sync");
}

void LlmModel::score_topk(const uint32_t* ids, int n, int first, int top_k, float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out)
{
    if (top_k < 1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > cfg_.vocab)
        throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [1, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                            "] and not above the vocabulary size " + std::to_string(cfg_.vocab));
    score_pass(ids, n, first, top_k);
    const size_t cnt = (size_t)(n - first);
    if (logprob_out) hip_check(hipMemcpyAsync(logprob_out, score_lp_, cnt * 4, hipMemcpyDeviceToHost, stream_), "D2H logprob");
    if (topk_ids_out) hip_check(hipMemcpyAsync(topk_ids_out, score_tk_ids_, cnt * top_k * 4, hipMemcpyDeviceToHost, stream_), "D2H top-k ids");
    if (topk_logprob_out)
        hip_check(hipMemcpyAsync(topk_logprob_out, score_tk_lp_, cnt * top_k * 4, hipMemcpyDeviceToHost, stream_), "D2H top-k logprob");
    hip_check(hipStreamSynchronize(stream_), "sync");
}

void LlmModel::last_hidden(float* out, int rows) const
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    hip_check(hipMemcpy(out, last_, (size_t)std::min(rows, last_rows_) * cfg_.hidden * sizeof(float), hipMemcpyDeviceToHost), "D2H hidden");
}

void LlmModel::kv_rows(int layer, int first, int rows, float* k_out, float* v_out) const
{
    if (layer < 0 || layer >= (int)layers_.size() || first < 0 || rows < 0 || first > cache_len_ || rows > cache_len_ - first)
        throw std::runtime_error("cache rows out of range");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    const size_t kv = (size_t)cfg_.kv_heads * cfg_.head_dim, off = (size_t)first * kv, bytes = (size_t)rows * kv * sizeof(float);
    const Layer& L = layers_[(size_t)layer];
    hip_check(hipMemcpy(k_out, L.k_cache + off, bytes, hipMemcpyDeviceToHost), "D2H k cache");
    hip_check(hipMemcpy(v_out, L.v_cache + off, bytes, hipMemcpyDeviceToHost), "D2H v cache");
}

void LlmModel::logits_to_host(float* out) const
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    hip_check(hipMemcpy(out, logits_, (size_t)cfg_.vocab * sizeof(float), hipMemcpyDeviceToHost), "D2H logits");
}

void LlmModel::enqueue_argmax(bool record)
{
    hip_check(launch_argmax(logits_, cfg_.vocab, best_, token_, record ? hist_ : nullptr, record ? count_ : nullptr,
                            record ? pos_ : nullptr, stream_), "argmax");
}

uint32_t LlmModel::argmax()
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    enqueue_argmax(false);
    int32_t t = 0;
    hip_check(hipMemcpyAsync(&t, token_, 4, hipMemcpyDeviceToHost, stream_), "D2H token");
    hip_check(hipStreamSynchronize(stream_), "sync");
    return (uint32_t)t;
}

hipGraphExec_t LlmModel::step_graph()
{
    if (graph_) return graph_;
    return graph_ = capture_graph(stream_, [&] {
        pass(reinterpret_cast<const uint32_t*>(token_), 1, true);
        enqueue_argmax(true);
    });
}

void LlmModel::ensure_constraint()
{
    if (cview_) return;
    cview_ = reinterpret_cast<ConstraintView*>(dalloc((sizeof(ConstraintView) + 3) / 4));
    crow_ = reinterpret_cast<ConstraintRow*>(dalloc((sizeof(ConstraintRow) + 3) / 4));
    cstate_log_ = reinterpret_cast<uint32_t*>(dalloc((size_t)hist_cap_));
}

hipGraphExec_t LlmModel::constrained_step_graph()
{
    if (cgraph_) return cgraph_;
    return cgraph_ = capture_graph(stream_, [&] {
        pass(reinterpret_cast<const uint32_t*>(token_), 1, true);
        hip_check(launch_constraint_apply(logits_, cfg_.vocab, 1, cfg_.vocab, cview_, crow_, stream_), "constraint apply");
        enqueue_argmax(true);
        hip_check(launch_constraint_advance(token_, 1, cview_, crow_, cstate_log_, count_, hist_cap_, stream_), "constraint advance");
    });
}

void LlmModel::ensure_grammar()
{
    if (gview_) return;
    gview_ = reinterpret_cast<GrammarView*>(dalloc((sizeof(GrammarView) + 3) / 4));
    grow_ = reinterpret_cast<GrammarRow*>(dalloc((sizeof(GrammarRow) + 3) / 4));
    gstate_log_ = reinterpret_cast<uint32_t*>(dalloc((size_t)hist_cap_));
    gdepth_log_ = reinterpret_cast<int32_t*>(dalloc((size_t)hist_cap_));
}

hipGraphExec_t LlmModel::grammar_step_graph()
{
    if (ggraph_) return ggraph_;
    return ggraph_ = capture_graph(stream_, [&] {
        pass(reinterpret_cast<const uint32_t*>(token_), 1, true);
        hip_check(launch_grammar_apply(logits_, cfg_.vocab, 1, cfg_.vocab, gview_, grow_, stream_), "grammar apply");
        enqueue_argmax(true);
        hip_check(launch_grammar_advance(token_, 1, gview_, grow_, gstate_log_, gdepth_log_, count_, hist_cap_, stream_), "grammar advance");
    });
}

void LlmModel::ensure_logprobs()
{
    if (lp_scratch_) return;
    lp_copy_ = dalloc((size_t)cfg_.vocab);
    lp_log_ = dalloc((size_t)hist_cap_);
    lp_tlp_log_ = dalloc((size_t)hist_cap_ * KJARNI_SCORE_TOPK_MAX);
    lp_ids_log_ = reinterpret_cast<uint32_t*>(dalloc((size_t)hist_cap_ * KJARNI_SCORE_TOPK_MAX));
    lp_tok_ = reinterpret_cast<int32_t*>(dalloc(4));
    lp_scratch_ = dalloc((token_logprob_scratch_bytes(1, cfg_.vocab) + 3) / 4);
}

void LlmModel::logprob_partial_on(const float* logits, int rows, const int32_t* live, int k, void* scratch, float* copy)
{
    TokenLogprobArgs a;
    a.logits = logits; a.ld = cfg_.vocab; a.rows = rows; a.vocab = cfg_.vocab; a.top_k = k; a.live = live; a.scratch = scratch;
    if (copy) { a.raw_copy = copy; a.ld_copy = cfg_.vocab; }
    hip_check(launch_token_logprob_partial(a, stream_), "token logprob partial");
}

void LlmModel::logprob_finish_on(const float* logits, int rows, const int32_t* live, int k, void* scratch, const float* raw, const int32_t* token,
                                 const int* count, int bias, int stride, float* lp, uint32_t* ids, float* tlp)
{
    TokenLogprobArgs a;
    a.logits = logits; a.ld = cfg_.vocab; a.rows = rows; a.vocab = cfg_.vocab; a.top_k = k; a.live = live; a.scratch = scratch;
    TokenLogprobRecord r;
    r.raw = raw; r.ld_raw = cfg_.vocab;
    r.tokens = token;
    r.count = count; r.index_bias = bias;
    r.rec_stride = stride; r.rec_cap = stride; r.slots = KJARNI_SCORE_TOPK_MAX;
    r.logprob = lp; r.topk_ids = ids; r.topk_logprob = tlp;
    hip_check(launch_token_logprob_finish(a, r, stream_), "token logprob finish");
}

void LlmModel::enqueue_logprob_partial(int k, bool copy) { logprob_partial_on(logits_, 1, nullptr, k, lp_scratch_, copy ? lp_copy_ : nullptr); }

void LlmModel::enqueue_logprob_finish(int k, bool from_copy, const int32_t* token, const int* count, int bias)
{
    logprob_finish_on(logits_, 1, nullptr, k, lp_scratch_, from_copy ? lp_copy_ : logits_, token, count, bias, hist_cap_, lp_log_, lp_ids_log_,
                      lp_tlp_log_);
}

// ---- lanes ----
void LlmModel::drop_lane_record_graphs(LaneBank& b)
{
    for (auto& g : b.lp_graphs) drop_graphs(g);
    for (auto& g : b.auto_graphs) drop_graphs(g);  // (the constrained chains hold the same lane buffers and capacity: they go where these go)
}

void LlmModel::drop_lane_graphs(LaneBank& b)
{
    drop_graphs(b.graphs);
    drop_lane_record_graphs(b);
}

void LlmModel::ensure_lane_logprobs(LaneBank& b)
{
    LaneLogs& L = b.logs;
    const int rows = b.max_lanes, stride = b.hist_stride;
    if (L.block && L.stride == stride) return;
    hip_check(hipStreamSynchronize(stream_), "sync");
    drop_lane_record_graphs(b);
    constexpr size_t S = KJARNI_SCORE_TOPK_MAX;
    auto pad = [](size_t floats) { return (floats + 63) & ~(size_t)63; };
    const size_t one = pad((size_t)rows * stride), many = pad((size_t)rows * stride * S), row = pad((size_t)cfg_.vocab);
    const size_t scratch = pad((token_logprob_scratch_bytes(rows, cfg_.vocab) + 3) / 4);
    void* fresh = arena_.alloc_own((one + 2 * many + row + scratch) * sizeof(float));
    if (L.block) arena_.free_own(L.block);
    L.block = fresh;
    float* at = static_cast<float*>(fresh);
    L.lp = at;
    L.tlp = at + one;
    L.ids = reinterpret_cast<uint32_t*>(at + one + many);
    L.copy = at + one + 2 * many;
    L.scratch = at + one + 2 * many + row;
    L.stride = stride;
}

void LlmModel::lane_logprobs_enqueue(LaneBank& b, int first, int rows, int k)
{
    const LaneLogs& L = b.logs;
    constexpr size_t S = KJARNI_SCORE_TOPK_MAX;
    const float* logits = b.logits + (size_t)first * cfg_.vocab;
    const int32_t* live = b.dev.live + first;
    const int* count = b.dev.count + first;
    logprob_partial_on(logits, rows, live, k, L.scratch, nullptr);
    logprob_finish_on(logits, rows, live, k, L.scratch, logits, nullptr, count, 0, L.stride, L.lp + (size_t)first * L.stride,
                      L.ids + (size_t)first * L.stride * S, L.tlp + (size_t)first * L.stride * S);
}

hipGraphExec_t LlmModel::lane_logprob_step_graph(LaneBank& b, int n, int k)
{
    hipGraphExec_t& g = b.lp_graphs[k > 1 ? 1 : 0][n];
    if (g) return g;
    return g = capture_graph(stream_, [&] {
        lane_step_enqueue(b, n);
        lane_logprobs_enqueue(b, 0, n, k);  // ahead of the pick: it reads the lanes' flags and counts as the step found them
        lane_pick_enqueue(b, n, 0, 1);
    });
}

// ---- constrained lanes ----
void LlmModel::ensure_lane_automata()
{
    if (lane_auto_) return;
    lane_auto_ = reinterpret_cast<LaneAutomatonTable*>(dalloc((sizeof(LaneAutomatonTable) + 3) / 4));
    lane_auto_host_ = std::make_unique<LaneAutomatonTable>();
    std::memset(lane_auto_host_.get(), 0, sizeof(LaneAutomatonTable));
    hip_check(hipMemcpy(lane_auto_, lane_auto_host_.get(), sizeof(LaneAutomatonTable), hipMemcpyHostToDevice), "H2D lane automata");
}

void LlmModel::lane_automaton_pick_enqueue(LaneBank& b, int first, int rows, int advance, bool records, int k)
{
    const LaneLogs& L = b.logs;
    constexpr size_t S = KJARNI_SCORE_TOPK_MAX;
    float* logits = b.logits;
    const float* part = logits + (size_t)first * cfg_.vocab;
    int32_t* live = b.dev.live;
    const int* count = b.dev.count;
    if (records) logprob_partial_on(part, rows, live + first, k, L.scratch, nullptr);  // the raw rows, ahead of the mask
    hip_check(launch_lane_automaton_apply(logits, cfg_.vocab, cfg_.vocab, rows, first, lane_auto_, live, stream_), "lane automaton apply");
    hip_check(launch_lane_automaton_pick(logits, cfg_.vocab, cfg_.vocab, rows, first, b.best, b.dev, b.hist, b.hist_stride, b.cap, advance,
                                         lane_auto_, stream_), "lane automaton pick");
    // the record of the lanes that picked, at index count - 1 (the pick has counted); the picked logit is an allowed one, which the
    // mask did not rewrite
    if (records)
        logprob_finish_on(part, rows, lane_auto_->fresh + first, k, L.scratch, part, lane_auto_->picked + first, count + first, -1, L.stride,
                          L.lp + (size_t)first * L.stride, L.ids + (size_t)first * L.stride * S, L.tlp + (size_t)first * L.stride * S);
}

hipGraphExec_t LlmModel::lane_automaton_step_graph(LaneBank& b, int n, bool records, int k)
{
    hipGraphExec_t& g = b.auto_graphs[!records ? 0 : k > 1 ? 2 : 1][n];
    if (g) return g;
    return g = capture_graph(stream_, [&] {
        lane_step_enqueue(b, n);
        lane_automaton_pick_enqueue(b, 0, n, 1, records, k);
    });
}

hipGraphExec_t LlmModel::logprob_step_graph(int kind, int k)
{
    hipGraphExec_t& g = lp_graphs_[kind][k > 1 ? 1 : 0];
    if (g) return g;
    return g = capture_graph(stream_, [&] {
        pass(reinterpret_cast<const uint32_t*>(token_), 1, true);
        enqueue_logprob_partial(k, kind != 0);
        if (kind == 1) hip_check(launch_constraint_apply(logits_, cfg_.vocab, 1, cfg_.vocab, cview_, crow_, stream_), "constraint apply");
        if (kind == 2) hip_check(launch_grammar_apply(logits_, cfg_.vocab, 1, cfg_.vocab, gview_, grow_, stream_), "grammar apply");
        enqueue_argmax(true);
        enqueue_logprob_finish(k, kind != 0, token_, count_, -1);  // (the pick is recorded at *count - 1)
        if (kind == 1) hip_check(launch_constraint_advance(token_, 1, cview_, crow_, cstate_log_, count_, hist_cap_, stream_), "constraint advance");
        if (kind == 2)
            hip_check(launch_grammar_advance(token_, 1, gview_, grow_, gstate_log_, gdepth_log_, count_, hist_cap_, stream_), "grammar advance");
    });
}

void LlmModel::fetch_logprobs(size_t first, size_t n, float* lp, uint32_t* ids, float* tlp)
{
    constexpr size_t S = KJARNI_SCORE_TOPK_MAX;
    hip_check(hipMemcpyAsync(lp + first, lp_log_ + first, n * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H logprobs");
    hip_check(hipMemcpyAsync(ids + first * S, lp_ids_log_ + first * S, n * S * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "D2H top-k ids");
    hip_check(hipMemcpyAsync(tlp + first * S, lp_tlp_log_ + first * S, n * S * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H top-k logprobs");
}

namespace {

// The record of one raw logits row on the host, in float32 (the loop with device sampling off): lse = max + log(sum exp(x - max)),
// the sum taken over blocks of 1 024 elements and then over the blocks; ids / lps [k] in the kernels' order (descending value,
// among equal values the larger id first, +0.0 == -0.0, NaN lowest).  A NaN at index 0 has key 0, the empty-slot marker: harmless,
// here as in the kernels, since an empty slot decodes to id 0 -- the same id.
float host_token_record(const float* x, size_t vocab, int k, uint32_t* ids, float* lps)
{
    const auto key = [](float v, size_t i) {
        uint32_t u;
        std::memcpy(&u, &v, 4);
        if (v == 0.0f) u = 0;
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        if (v != v) u = 0;
        return ((uint64_t)u << 32) | (uint32_t)i;
    };
    uint64_t lst[KJARNI_SCORE_TOPK_MAX + 1] = {};
    float mx = -INFINITY;
    for (size_t i = 0; i < vocab; ++i) {
        mx = std::fmax(mx, x[i]);
        const uint64_t kk = key(x[i], i);
        int j = k;
        for (; j > 0 && kk > lst[j - 1]; --j) lst[j] = lst[j - 1];
        lst[j] = kk;
    }
    float sum = 0.0f;
    for (size_t b = 0; b < vocab; b += 1024) {
        float part = 0.0f;
        for (size_t i = b; i < std::min(vocab, b + 1024); ++i) part += std::exp(x[i] - mx);
        sum += part;
    }
    const float lse = mx + std::log(sum);
    for (int j = 0; j < k; ++j) {
        ids[j] = (uint32_t)(lst[j] & 0xFFFFFFFFull);
        lps[j] = x[ids[j]] - lse;
    }
    return lse;
}

// What generate() needs of the host's copy of the automaton, regular (a DeviceConstraint: one state) or with a stack (a
// DeviceGrammar: a configuration).  The loop below is written once against it.
struct AutomatonCursor {
    const DeviceConstraint* con = nullptr;
    const DeviceGrammar* gram = nullptr;
    uint32_t hq = 0;   // under a constraint
    GrammarConfig hc;  // under a grammar

    explicit operator bool() const { return con || gram; }
    uint32_t state() const { return con ? hq : hc.state; }
    int32_t depth() const { return con ? 0 : hc.depth; }
    bool accepting() const { return con ? con->dfa().accepting[hq] != 0 : gram->grammar().accepted(hc); }
    bool closed() const { return con ? con->dfa().closed[hq] != 0 : gram->grammar().closed(hc); }
    // Would the mask leave token t (no stop id) as it is?
    bool allows(uint32_t t) const
    {
        if (con) return con->allows(hq, t);
        GrammarConfig c = hc;
        return gram->step_token(&c, t);
    }
    // Moves by token t; false (and no move) when the mask does not allow it.
    bool step(uint32_t t)
    {
        if (con) {
            const uint32_t next = con->allows(hq, t) ? con->step_token(hq, t) : (uint32_t)kConstraintDead;
            if (next == kConstraintDead) return false;
            hq = next;
            return true;
        }
        GrammarConfig c = hc;
        if (!gram->step_token(&c, t)) return false;
        hc = c;
        return true;
    }
};

}  // namespace

void LlmModel::ensure_host_logits()
{
    if (!host_logits_) hip_check(hipHostMalloc((void**)&host_logits_, (size_t)cfg_.vocab * sizeof(float), hipHostMallocDefault), "hipHostMalloc");
}

void LlmModel::ensure_sampling()
{
    if (samp_scratch_) return;
    const size_t vocab = (size_t)cfg_.vocab;
    const size_t out_bytes = sizeof(SampleHeader) + (size_t)kCandCap * sizeof(SampleCandidate);
    samp_scratch_ = dalloc((sample_scratch_bytes() + 3) / 4);
    hip_check(hipMemset(samp_scratch_, 0, sample_scratch_bytes()), "memset");
    samp_out_ = reinterpret_cast<uint8_t*>(dalloc((out_bytes + 3) / 4));
    hip_check(hipMemset(samp_out_, 0, out_bytes), "memset");
    hip_check(hipHostMalloc((void**)&samp_host_, out_bytes, hipHostMallocDefault), "hipHostMalloc");
    samp_tokens_ = reinterpret_cast<int32_t*>(dalloc((size_t)cache_cap_ + 16));
    samp_distinct_ = reinterpret_cast<int32_t*>(dalloc((size_t)cache_cap_ + 16));
    samp_counts_ = reinterpret_cast<int*>(dalloc(vocab));
    samp_ndistinct_ = reinterpret_cast<int*>(dalloc(4));
}

std::vector<uint32_t> LlmModel::generate(const std::vector<uint32_t>& prompt, size_t max_new_tokens, float repetition_penalty,
                                         int no_repeat_ngram, const std::function<bool(uint32_t)>& on_token)
{
    GenerateOptions o;
    o.max_new_tokens = max_new_tokens;
    o.repetition_penalty = repetition_penalty;
    o.no_repeat_ngram = no_repeat_ngram;
    return generate(prompt, o, on_token);
}

std::vector<uint32_t> LlmModel::generate(const std::vector<uint32_t>& prompt, const GenerateOptions& opt,
                                         const std::function<bool(uint32_t)>& on_token)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (prompt.empty()) throw std::runtime_error("cannot generate from empty prompt");
    if ((int)prompt.size() > cache_cap_) throw std::runtime_error("prompt does not fit the context");
    if (opt.sample && !opt.uniform) throw std::runtime_error("sampling needs a uniform source");
    if (opt.logprobs < -1 || opt.logprobs > KJARNI_SCORE_TOPK_MAX || opt.logprobs > cfg_.vocab)
        throw InvalidConfig("top_k (" + std::to_string(opt.logprobs) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                            "] and not above the vocabulary (" + std::to_string(cfg_.vocab) + ")");
    const DeviceConstraint* con = opt.constraint;
    if (con) {  // everything that can be refused is refused before any GPU work
        if (con->device() != device_)
            throw InvalidConfig("the constraint lives on device " + std::to_string(con->device()) + ", the model on device " + std::to_string(device_));
        if (con->vocab() != cfg_.vocab)
            throw InvalidConfig("the constraint's token table has " + std::to_string(con->vocab()) + " tokens, the model's vocabulary " +
                                std::to_string(cfg_.vocab));
        con->check_states(opt.stop_ids.empty() ? cfg_.eos_ids : opt.stop_ids);
    }
    const DeviceGrammar* gram = opt.grammar;
    if (gram) {
        if (con) throw InvalidConfig("a call takes a constraint or a grammar, not both");
        if (gram->device() != device_)
            throw InvalidConfig("the grammar lives on device " + std::to_string(gram->device()) + ", the model on device " + std::to_string(device_));
        if (gram->vocab() != cfg_.vocab)
            throw InvalidConfig("the grammar's token table has " + std::to_string(gram->vocab()) + " tokens, the model's vocabulary " +
                                std::to_string(cfg_.vocab));
        gram->check_states(opt.stop_ids.empty() ? cfg_.eos_ids : opt.stop_ids);
    }
    begin_sequence(prompt);
    std::vector<uint32_t> out;
    GenerationRun run(prompt, opt, (size_t)cache_cap_, cfg_.eos_ids, out);
    // Log-probabilities: off unless asked for and given a sink.  lpk: the width the device computes (llm.h).
    TokenLogprobs* const sink = opt.logprobs >= 0 ? opt.logprob_sink : nullptr;
    const bool lp = sink != nullptr;
    const int lpk = opt.logprobs <= 1 ? 1 : std::min(KJARNI_SCORE_TOPK_MAX, cfg_.vocab);
    constexpr size_t kSlots = KJARNI_SCORE_TOPK_MAX;
    std::vector<float> lp_host, lp_tlp_host;
    std::vector<uint32_t> lp_ids_host;
    if (lp) {
        sink->clear(opt.logprobs);
        ensure_logprobs();
        lp_host.resize((size_t)hist_cap_);
        lp_ids_host.resize((size_t)hist_cap_ * kSlots);
        lp_tlp_host.resize((size_t)hist_cap_ * kSlots);
    }
    const auto push_record = [&](size_t i) { sink->push(lp_host[i], lp_ids_host.data() + i * kSlots, lp_tlp_host.data() + i * kSlots); };
    // The constrained run: the host walks its own copy of the automaton over the tokens it takes (`hq`), the device holds the
    // state the kernels read (crow_).  take() is run.accept() under the constraint: a stop id ends the run (complete when the
    // state is accepting), any other token moves hq, and a closed state ends the run behind the token.
    // Under a grammar the same holds with "configuration" for "state" (grow_, the kernels of grammar_kernels.h).
    ConstraintOutcome outcome;
    AutomatonCursor cur;
    cur.con = con;
    cur.gram = gram;
    cur.hq = con ? con->dfa().start : 0;
    const uint32_t hq = cur.hq;
    if (gram) {
        ensure_grammar();
        const GrammarView view = gram->view(run.stops);
        GrammarRow row = {};
        hip_check(hipMemcpyAsync(gview_, &view, sizeof(view), hipMemcpyHostToDevice, stream_), "H2D grammar view");
        hip_check(hipMemcpyAsync(grow_, &row, sizeof(row), hipMemcpyHostToDevice, stream_), "H2D grammar state");
        hip_check(hipStreamSynchronize(stream_), "sync");  // (both sources are locals)
    }
    const auto launch_apply = [&] {
        if (con) hip_check(launch_constraint_apply(logits_, (int64_t)cfg_.vocab, 1, cfg_.vocab, cview_, crow_, stream_), "constraint apply");
        if (gram) hip_check(launch_grammar_apply(logits_, (int64_t)cfg_.vocab, 1, cfg_.vocab, gview_, grow_, stream_), "grammar apply");
    };
    const auto launch_advance = [&](bool logged) {
        if (con)
            hip_check(launch_constraint_advance(token_, 1, cview_, crow_, logged ? cstate_log_ : nullptr, logged ? count_ : nullptr,
                                                logged ? hist_cap_ : 0, stream_), "constraint advance");
        if (gram)
            hip_check(launch_grammar_advance(token_, 1, gview_, grow_, logged ? gstate_log_ : nullptr, logged ? gdepth_log_ : nullptr,
                                             logged ? count_ : nullptr, logged ? hist_cap_ : 0, stream_), "grammar advance");
    };
    // The device's row after the run: its state (and depth), and whether any step picked a masked token.
    const auto read_device_row = [&](bool state_too) {
        if (con) {
            ConstraintRow row = {};
            hip_check(hipMemcpyAsync(&row, crow_, sizeof(row), hipMemcpyDeviceToHost, stream_), "D2H constraint state");
            hip_check(hipStreamSynchronize(stream_), "sync");
            if (state_too) outcome.device_state = row.state;
            outcome.violated = outcome.violated || row.violated != 0;
        }
        if (gram) {
            GrammarRow row = {};
            hip_check(hipMemcpyAsync(&row, grow_, 16, hipMemcpyDeviceToHost, stream_), "D2H grammar state");  // (state, depth, done, violated)
            hip_check(hipStreamSynchronize(stream_), "sync");
            if (state_too) {
                outcome.device_state = row.state;
                outcome.device_depth = row.depth;
            }
            outcome.violated = outcome.violated || row.violated != 0;
        }
    };
    if (con) {
        ensure_constraint();
        const ConstraintView view = con->view(run.stops);
        const ConstraintRow row = {hq, 0, 0, 0};
        hip_check(hipMemcpyAsync(cview_, &view, sizeof(view), hipMemcpyHostToDevice, stream_), "H2D constraint view");
        hip_check(hipMemcpyAsync(crow_, &row, sizeof(row), hipMemcpyHostToDevice, stream_), "H2D constraint state");
        hip_check(hipStreamSynchronize(stream_), "sync");  // (both sources are locals)
        outcome.device_state = hq;
    }
    const auto take = [&](uint32_t tok) -> bool {
        if (!cur) return run.accept(tok, on_token);
        if (!run.wants_token()) {
            run.done = true;
            return false;
        }
        if (run.is_stop(tok)) {
            (cur.accepting() ? outcome.complete : outcome.violated) = true;
            run.done = true;
            return false;
        }
        if (!cur.step(tok)) {
            outcome.violated = true;
            run.done = true;
            return false;
        }
        const bool taken = run.accept(tok, on_token);
        if (cur.closed()) outcome.complete = run.done = true;
        return taken;
    };
    const auto finish = [&] {
        if (!cur) return;
        outcome.final_state = cur.state();
        outcome.final_depth = cur.depth();
        outcome.accepted = cur.accepting();
        if (opt.constraint_outcome) *opt.constraint_outcome = outcome;
    };
    const float repetition_penalty = opt.repetition_penalty;
    const int no_repeat_ngram = opt.no_repeat_ngram;
    const bool processors = repetition_penalty != 1.0f || no_repeat_ngram > 0;
    const size_t vocab = (size_t)cfg_.vocab;
    // The two loops below decide a token from the logits of the last step, then run the next step on it: the replayed graph
    // of the greedy loop, which reads its input token from token_ (overwritten here with the host's choice; the graph's own
    // argmax result is ignored) and advances position and key count on the device.
    hipGraphExec_t exec = nullptr;
    const auto feed = [&](uint32_t next) {
        if (!exec) exec = step_graph();
        const int32_t tok = (int32_t)next;
        hip_check(hipMemcpyAsync(token_, &tok, sizeof(tok), hipMemcpyHostToDevice, stream_), "H2D token");
        if (processors && device_sampling_) {
            int32_t* slot = samp_tokens_ + (run.all.size() - 1);
            hip_check(hipMemcpyAsync(slot, &tok, sizeof(tok), hipMemcpyHostToDevice, stream_), "H2D history");
            hip_check(launch_token_counts(slot, 1, (int)vocab, samp_counts_, samp_distinct_, samp_ndistinct_, stream_), "token counts");
        }
        hip_check(hipGraphLaunch(exec, stream_), "graph launch");
        cache_len_ += 1;
    };

    if ((opt.sample || processors) && device_sampling_) {
        // Logits processors and sampling (generator.rs:331-343), with everything that is O(vocab) on the device
        // (llm_kernels.hip): the processors edit the logits where the vocabulary head left them; for a sampled token three
        // small launches cut the vocabulary down to the candidates within reach of the filters and sum the exponentials,
        // and the host receives a 32-byte header + a few hundred (token, logit) pairs instead of 4 x vocab bytes.  It
        // finishes top-k / top-p / min-p / temperature / the draw on them exactly as the reference does on the full array
        // (sampling.cpp); when the candidates cannot decide (rare: a crossing within the rounding of the device's sum, a
        // nearly flat distribution) it fetches the logits -- already processed -- and runs the full-array path.
        ensure_sampling();
        if (opt.sample) ensure_host_logits();
        SampleHeader* header_dev = reinterpret_cast<SampleHeader*>(samp_out_);
        SampleCandidate* cand_dev = reinterpret_cast<SampleCandidate*>(samp_out_ + sizeof(SampleHeader));
        const SampleHeader* header = reinterpret_cast<const SampleHeader*>(samp_host_);
        const SampleCandidate* cand = reinterpret_cast<const SampleCandidate*>(samp_host_ + sizeof(SampleHeader));
        if (processors) {
            begin_token_history(samp_tokens_, run.all.data(), run.all.size(), samp_counts_, samp_distinct_, samp_ndistinct_);
            hip_check(hipStreamSynchronize(stream_), "sync");  // (`all` grows below: the copy must have read it)
        }
        int skip_candidates = 0;
        const bool edits = cur || processors;  // logits_ is edited in place before the token is known: the record reads the copy
        while (run.wants_token()) {
            if (lp) enqueue_logprob_partial(lpk, edits);
            launch_apply();
            if (processors)
                hip_check(launch_logits_processors(logits_, (int)vocab, samp_tokens_, (int)run.all.size(), samp_counts_, samp_distinct_,
                                                   samp_ndistinct_, repetition_penalty, no_repeat_ngram, stream_), "logits processors");
            uint32_t next;
            if (opt.sample) {
                // A distribution the candidates could not decide (nearly flat: top-p reaches through most of the vocabulary) rarely
                // becomes decidable on the next token: after a miss the cut is not attempted for a few tokens.
                const bool attempt = skip_candidates == 0;
                if (!attempt) --skip_candidates;
                const size_t first = sizeof(SampleHeader) + (size_t)kCandFirst * sizeof(SampleCandidate);
                if (attempt) {
                    hip_check(launch_sample_candidates(logits_, (int)vocab, opt.sampling.top_k, opt.sampling.top_p, opt.sampling.min_p,
                                                       samp_scratch_, header_dev, cand_dev, kCandCap, stream_), "sample candidates");
                    hip_check(hipMemcpyAsync(samp_host_, samp_out_, first, hipMemcpyDeviceToHost, stream_), "D2H candidates");
                    hip_check(hipStreamSynchronize(stream_), "sync");
                }
                bool decided = false;
                next = sample_row(attempt ? header : nullptr, kCandFirst, kCandCap, [&](size_t i) -> const SampleCandidate& { return cand[i]; },
                                  [&](size_t n) {
                                      hip_check(hipMemcpyAsync(samp_host_ + first, samp_out_ + first, (n - kCandFirst) * sizeof(SampleCandidate),
                                                               hipMemcpyDeviceToHost, stream_), "D2H candidates");
                                      hip_check(hipStreamSynchronize(stream_), "sync");
                                  },
                                  logits_, opt.sampling, opt.uniform(), &decided);  // (the processors already ran, on the device)
                if (!decided && attempt) skip_candidates = 8;
            } else {  // greedy on processed logits: the device's argmax (last maximum wins), four bytes back
                enqueue_argmax(false);
                int32_t t = 0;
                hip_check(hipMemcpyAsync(&t, token_, sizeof(t), hipMemcpyDeviceToHost, stream_), "D2H token");
                hip_check(hipStreamSynchronize(stream_), "sync");
                next = (uint32_t)t;
                ++tokens_from_candidates_;
            }
            // LastToken::Fed: one step per emitted token, the last of max_new_tokens included -- under an explicit max_len past
            // prompt + max_new_tokens; with the default max_len that token fills context_limit and is not fed
            if (!take(next)) break;
            if (lp) {  // the record of the emitted token, fed or not, at its index in the output
                const int32_t tok = (int32_t)next;
                hip_check(hipMemcpyAsync(lp_tok_, &tok, sizeof(tok), hipMemcpyHostToDevice, stream_), "H2D token");
                enqueue_logprob_finish(lpk, edits, lp_tok_, nullptr, (int)out.size() - 1);
            }
            if (cur) {  // the device's automaton takes the host's choice (fed or not, so that it ends where the host's does)
                const int32_t tok = (int32_t)next;
                hip_check(hipMemcpyAsync(token_, &tok, sizeof(tok), hipMemcpyHostToDevice, stream_), "H2D token");
                launch_advance(false);
            }
            if (outcome.complete || !run.feeds_accepted(LastToken::Fed)) break;  // (a closed state: nothing follows the token)
            feed(next);
        }
        read_device_row(true);
        if (lp && !out.empty()) {
            fetch_logprobs(0, out.size(), lp_host.data(), lp_ids_host.data(), lp_tlp_host.data());
            hip_check(hipStreamSynchronize(stream_), "sync");
            for (size_t i = 0; i < out.size(); ++i) push_record(i);
        }
        finish();
        leave_resident(run.all);
        return out;
    }

    if (opt.sample || processors) {
        // (device sampling switched off: the checker path of the tests)
        // Logits processors and sampling work on the host copy of the logits (generator.rs:331-343): one pass per token.
        // The logits land in a pinned host buffer (one async copy per token at full PCIe rate).
        ensure_host_logits();
        float* lg = host_logits_;
        std::vector<float> probs, lp_raw;
        std::vector<uint32_t> ids;
        while (run.wants_token()) {
            hip_check(hipMemcpyAsync(lg, logits_, vocab * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H logits");
            hip_check(hipStreamSynchronize(stream_), "sync");
            float rec_lse = 0.0f, rec_lps[kSlots] = {};
            uint32_t rec_ids[kSlots] = {};
            if (lp) {  // the record from the raw row, before anything below edits it
                rec_lse = host_token_record(lg, vocab, opt.logprobs, rec_ids, rec_lps);
                lp_raw.assign(lg, lg + vocab);  // (the mask and the processors edit lg in place; the chosen token's raw logit is read below)
            }
            if (cur) {  // the same mask from the host's automaton and token table
                const bool accepting = cur.accepting();
                for (size_t v = 0; v < vocab; ++v)
                    if (!(run.is_stop((uint32_t)v) ? accepting : cur.allows((uint32_t)v))) lg[v] = -INFINITY;
            }
            apply_repetition_penalty(lg, vocab, run.all, repetition_penalty);
            if (no_repeat_ngram > 0) apply_no_repeat_ngram(lg, vocab, run.all, (size_t)no_repeat_ngram);
            uint32_t next;
            if (opt.sample) {
                sampling_distribution(lg, vocab, opt.sampling, ids, probs);
                next = sample_from_distribution(ids, probs, opt.uniform(), vocab);
            } else {
                next = argmax_last(lg, vocab);
            }
            // LastToken::Fed, as the loop above
            const bool taken = take(next);
            if (taken && lp) sink->push(lp_raw[next] - rec_lse, rec_ids, rec_lps);
            if (!taken || outcome.complete || !run.feeds_accepted(LastToken::Fed)) break;
            feed(next);
        }
        outcome.device_state = cur.state();  // (no device automaton on this path)
        outcome.device_depth = cur.depth();
        finish();
        leave_resident(run.all);
        return out;
    }

    // Plain greedy: token, position and key count stay on the device; one graph replay per token, the host
    // looks every few steps.  Tokens computed past a stop token / a stop request are discarded.  The device feeds itself:
    // a burst is sized by what is left of max_new_tokens, so the last token of max_new_tokens is not fed (LastToken::NotFed).
    // Constrained: the chain is pass -> apply -> argmax -> advance; the host steps its own automaton per drained token and ends the
    // run at a stop id, a closed state or the limits, discarding what the device ran past that point as it does past a stop id.
    if (lp) enqueue_logprob_partial(lpk, (bool)cur);
    launch_apply();
    enqueue_argmax(true);
    if (lp) enqueue_logprob_finish(lpk, (bool)cur, token_, count_, -1);
    launch_advance(true);
    hip_check(hipMemcpyAsync(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    std::vector<int32_t> hist((size_t)hist_cap_);
    std::vector<uint32_t> states(cur ? (size_t)hist_cap_ : 0);
    std::vector<int32_t> depths(gram ? (size_t)hist_cap_ : 0);
    size_t produced = 0, seen = 0;
    auto drain = [&](size_t upto) {
        for (; seen < upto && !run.done; ++seen) {
            if (!take((uint32_t)hist[seen])) continue;
            if (lp) push_record(seen);
            if (cur) {
                outcome.device_state = states[seen];
                if (gram) outcome.device_depth = depths[seen];
            }
        }
    };
    const auto fetch = [&](size_t first, size_t n) {  // the picks [first, first + n) and, constrained, the states behind them
        hip_check(hipMemcpyAsync(hist.data() + first, hist_ + first, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream_), "D2H tokens");
        if (con)
            hip_check(hipMemcpyAsync(states.data() + first, cstate_log_ + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "D2H states");
        if (gram) {
            hip_check(hipMemcpyAsync(states.data() + first, gstate_log_ + first, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "D2H states");
            hip_check(hipMemcpyAsync(depths.data() + first, gdepth_log_ + first, n * sizeof(int32_t), hipMemcpyDeviceToHost, stream_), "D2H depths");
        }
        if (lp) fetch_logprobs(first, n, lp_host.data(), lp_ids_host.data(), lp_tlp_host.data());
        hip_check(hipStreamSynchronize(stream_), "sync");
    };
    fetch(0, 1);
    produced = 1;
    drain(1);
    if (!run.done)
        exec = lp ? logprob_step_graph(con ? 1 : gram ? 2 : 0, lpk) : con ? constrained_step_graph() : gram ? grammar_step_graph() : step_graph();
    const size_t burst = on_token ? 4 : 16;
    while (!run.done) {
        size_t steps = std::min(burst, run.max_new - out.size());
        steps = std::min(steps, (size_t)cache_cap_ - (size_t)cache_len_);
        if (steps == 0) break;
        for (size_t i = 0; i < steps; ++i) hip_check(hipGraphLaunch(exec, stream_), "graph launch");
        fetch(produced, steps);
        produced += steps;
        cache_len_ += (int)steps;
        drain(produced);
    }
    read_device_row(false);  // violated alone (steps past the run's end included: they pick under the mask too)
    finish();
    leave_resident(run.all);  // (the burst's rows past the last emitted token stay behind cache_len_, uncounted)
    return out;
}

// The history so far = the given tokens: their counts and the list of the distinct ones.
void LlmModel::begin_token_history(int32_t* tokens_dev, const uint32_t* host, size_t n, int* counts, int32_t* distinct, int* ndistinct)
{
    const int vocab = cfg_.vocab;
    hip_check(hipMemsetAsync(counts, 0, (size_t)vocab * sizeof(int), stream_), "memset counts");
    hip_check(hipMemsetAsync(ndistinct, 0, sizeof(int), stream_), "memset");
    if (host) hip_check(hipMemcpyAsync(tokens_dev, host, n * sizeof(int32_t), hipMemcpyHostToDevice, stream_), "H2D history");
    hip_check(launch_token_counts(tokens_dev, (int)n, vocab, counts, distinct, ndistinct, stream_), "token counts");
}

template <class Cand, class FetchRest>
uint32_t LlmModel::sample_row(const SampleHeader* header, int first, int capacity, Cand&& cand, FetchRest&& fetch_rest, const float* logits_dev,
                              const SamplingParams& params, float uniform, bool* decided_out)
{
    const size_t vocab = (size_t)cfg_.vocab;
    bool decided = false;
    if (header && !header->overflow && header->count <= (uint32_t)capacity) {
        const size_t n = header->count;
        if (n > (size_t)first) fetch_rest(n);  // (they were not part of the step's copy)
        row_cids_.resize(n);
        row_cvals_.resize(n);
        for (size_t i = 0; i < n; ++i) {
            const SampleCandidate& c = cand(i);
            row_cids_[i] = c.token;
            row_cvals_[i] = c.logit;
        }
        decided = sampling_distribution_candidates(row_cids_.data(), row_cvals_.data(), n, header->mx, header->floor, header->sum, vocab, params,
                                                   row_ids_, row_probs_);
    }
    if (decided) {
        ++tokens_from_candidates_;
    } else {
        ++tokens_from_logits_;
        hip_check(hipMemcpyAsync(host_logits_, logits_dev, vocab * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H logits");
        hip_check(hipStreamSynchronize(stream_), "sync");
        sampling_distribution(host_logits_, vocab, params, row_ids_, row_probs_);
    }
    if (decided_out) *decided_out = decided;
    return sample_from_distribution(row_ids_, row_probs_, uniform, vocab);
}


// ---------------------------------------------------------------------------------------------------------------------
// Lanes: sequences decoded in lock step, in two banks (LaneBank) that one loop, generate_on_lanes(), schedules: 1..8 lanes on
// the GEMV kernels (lane_step) and 9..64 on the prompt GEMM (wide_step_enqueue, further down).  A lane is one sequence with its
// own KV cache (lane-major: lane l of a layer sits at base + l * alloc_cap * kv) and its own position; token, position, live
// flag, pick count and stop rules of every lane live on the device (LlmLaneState / LlmWideState), so a step is one linear chain
// of launches on one stream that replays as a captured graph.  The lanes bank's: embed (GPT-2: + wpe[pos[lane]]) -> per layer
// [norm + Q|K|V into the staging rows -> rotate Q, rotate K and scatter K / V to row pos[lane] of the lane's cache -> ragged
// attention (pos[lane] + 1 keys) + merge -> o-proj + residual -> norm + gate/up (c_fc + GELU) -> down + residual] -> final
// norm -> vocabulary head [lanes, vocab] -> lane pick.  Seven launches per layer, two more than the one-token step (which
// fuses the rotation into the projection and the merge into the o-proj).

void LlmModel::ensure_lane_bank(LaneBank& b, int lanes, int lane_context)
{
    if (lanes < b.min_lanes || lanes > b.max_lanes) throw InvalidConfig(b.range_error);
    const LlmConfig& c = cfg_;
    const int cap = lane_context <= 0 ? cache_cap_ : std::min(cache_cap_, lane_context);
    if (b.wide) {  // what the wide step alone asks of the checkpoint
        if (quant_ && !fp8_mc_)  // (fp8_ implies quant_; fp8_mc_ implies fp8_: with the switch on, the FP8 prompt GEMM reads the codes)
            throw InvalidConfig(std::string("more than 8 lanes do not take a ") + (fp8_ ? "FP8" : "quantized (GGUF)") +
                                " checkpoint: the prompt GEMM would dequantize every matrix in every step (8 lanes or fewer run it)");
        if (!rows_geometry(c) || !decode_attention_accepts(c.head_dim, splits_, cap, 1, true, true, false))
            throw InvalidConfig("more than 8 lanes need hidden, heads * head_dim and intermediate_size multiples of 32 and a head_dim that is a "
                                "multiple of 4 dividing 1024 (8 lanes or fewer run other shapes)");
        ensure_prompt_workspace();
    }
    const size_t kv = (size_t)(gpt2_ ? c.hidden : c.kv_heads * c.head_dim), vocab = (size_t)c.vocab;
    if (!b.state) {  // what the layout's width sizes: allocated once
        b.state = dalloc((b.state_bytes + 3) / 4);
        b.dev = LaneStateRef::at(b.state, b.width);
        b.mirror = std::make_unique<int32_t[]>(b.state_bytes / sizeof(int32_t));
        b.host = LaneStateRef::at(b.mirror.get(), b.width);
        b.best = reinterpret_cast<unsigned long long*>(dalloc(2 * (size_t)b.width));
        hip_check(hipMemset(b.best, 0, sizeof(unsigned long long) * b.width), "memset");
        b.copy_table = reinterpret_cast<LlmKvCopyPair*>(dalloc((layers_.size() * sizeof(LlmKvCopyPair) + 3) / 4));
    }
    if (lanes > b.alloc || cap > b.alloc_cap) {
        hip_check(hipStreamSynchronize(stream_), "sync");
        drop_lane_graphs(b);
        // one allocation of its own, sized by the lanes and the rows asked for, replaced (and the old one freed) when either grows.
        // Kept as they are: the lanes bank's step works in the single-sequence att_scratch_, ctx_, h_ and last_ (layer_finish() and
        // head() are pass()'s), the wide bank's in the prompt workspace with an attention scratch of its own, carved here.
        const size_t nl = (size_t)std::max(lanes, b.alloc), nc = (size_t)std::max(cap, b.alloc_cap), stride = nc + 16;
        auto pad = [](size_t floats) { return (floats + 63) & ~(size_t)63; };
        const size_t per_cache = pad(nl * nc * kv), qkv = pad(nl * ((size_t)c.q_dim() + 2 * kv)), logits = pad(nl * vocab);
        const size_t att = b.wide ? pad(decode_attention_scratch_floats((int)nl, c.heads, c.head_dim, splits_)) : 0, hist = pad(nl * stride);
        const size_t floats = 2 * layers_.size() * per_cache + qkv + 2 * logits + att + 3 * hist + pad(nl);
        void* fresh = arena_.alloc_own(floats * sizeof(float));
        if (b.block) arena_.free_own(b.block);
        b.block = fresh;
        float* at = static_cast<float*>(fresh);
        auto take = [&](size_t n) {
            float* p = at;
            at += n;
            return p;
        };
        b.k.assign(layers_.size(), nullptr);
        b.v.assign(layers_.size(), nullptr);
        for (size_t i = 0; i < layers_.size(); ++i) {
            b.k[i] = take(per_cache);
            b.v[i] = take(per_cache);
        }
        b.qkv = take(qkv);
        b.logits = take(logits);
        b.pcounts = reinterpret_cast<int*>(take(logits));
        b.att = take(att);
        b.hist_stride = (int)stride;
        b.hist = reinterpret_cast<int32_t*>(take(hist));
        b.ptok = reinterpret_cast<int32_t*>(take(hist));
        b.pdistinct = reinterpret_cast<int32_t*>(take(hist));
        b.pndistinct = reinterpret_cast<int*>(take(pad(nl)));
        b.alloc = (int)nl;
        b.alloc_cap = (int)nc;
        // the shared-prefix copy reads its pointers from the device: (main K, lane-0 K, main V, lane-0 V) per layer
        std::vector<LlmKvCopyPair> pairs(layers_.size());
        for (size_t i = 0; i < layers_.size(); ++i) pairs[i] = {layers_[i].k_cache, b.k[i], layers_[i].v_cache, b.v[i]};
        hip_check(hipMemcpy(b.copy_table, pairs.data(), pairs.size() * sizeof(LlmKvCopyPair), hipMemcpyHostToDevice), "H2D copy table");
    }
    if (cap != b.cap) drop_lane_graphs(b);  // (the capacity is an argument of the captured launches)
    b.lanes = lanes;
    b.cap = cap;
    std::memset(b.mirror.get(), 0, b.state_bytes);
    std::fill(b.len, b.len + kWideLanes, 0);
    lane_state_to_device(b);
}

void LlmModel::lane_state_to_device(LaneBank& b)
{
    hip_check(hipMemcpyAsync(b.state, b.mirror.get(), b.state_bytes, hipMemcpyHostToDevice, stream_), "H2D lane state");
    hip_check(hipStreamSynchronize(stream_), "sync");  // (the mirror is edited again right away)
}

void LlmModel::lane_state_from_device(LaneBank& b)
{
    hip_check(hipMemcpyAsync(b.mirror.get(), b.state, b.state_bytes, hipMemcpyDeviceToHost, stream_), "D2H lane state");
    hip_check(hipStreamSynchronize(stream_), "sync");
}

void LlmModel::lanes_begin(Bank bank, int lanes, int lane_context)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    LaneBank& b = bank_of(bank);
    ensure_lane_bank(b, lanes == 0 ? b.max_lanes : lanes, lane_context);
}

void LlmModel::lane_prefill(Bank bank, int lane, const uint32_t* ids, int n) { lane_prefill_at(bank_of(bank), lane, 0, ids, n); }

// Rows [0, s) of every layer's K and V, single-sequence cache -> lane, in one launch on the model's stream.
void LlmModel::lane_copy_prefix(LaneBank& b, int lane, int s)
{
    if (lane < 0 || lane >= b.lanes) throw std::runtime_error("no such lane");
    if (s < 0 || s > cache_len_ || s > b.cap) throw std::runtime_error("shared prefix out of range");
    const int64_t kv = gpt2_ ? cfg_.hidden : cfg_.kv_heads * cfg_.head_dim;
    hip_check(launch_kv_prefix_copy(b.copy_table, (int)layers_.size(), (int64_t)lane * b.alloc_cap * kv, (int64_t)s * kv, stream_), "prefix copy");
}

void LlmModel::lane_prefill_shared(Bank bank, int lane, int s, const uint32_t* ids, int n) { lane_prefill_shared(bank_of(bank), lane, s, ids, n); }

void LlmModel::lane_prefill_shared(LaneBank& b, int lane, int s, const uint32_t* ids, int n)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (lane < 0 || lane >= b.lanes) throw std::runtime_error("no such lane");
    if (n < 1) throw std::runtime_error("cannot generate from empty prompt");
    if (s < 0 || s > cache_len_) throw std::runtime_error("shared prefix out of range");
    if ((int64_t)s + n > b.cap) throw std::runtime_error("prompt does not fit the lane");
    lane_copy_prefix(b, lane, s);
    lane_prefill_at(b, lane, s, ids, n);
}

void LlmModel::lane_prefill_at(LaneBank& b, int lane, int base, const uint32_t* ids, int n)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (lane < 0 || lane >= b.lanes) throw std::runtime_error("no such lane");
    if (n < 1) throw std::runtime_error("cannot generate from empty prompt");
    if (base < 0 || (int64_t)base + n > b.cap) throw std::runtime_error("prompt does not fit the lane");
    const size_t kv = (size_t)(gpt2_ ? cfg_.hidden : cfg_.kv_heads * cfg_.head_dim), off = (size_t)lane * b.alloc_cap * kv;
    std::vector<std::pair<float*, float*>> saved(layers_.size());
    const int saved_len = cache_len_, saved_cap = cache_cap_, saved_rows = last_rows_;
    const size_t saved_resident = resident_.size();
    for (size_t i = 0; i < layers_.size(); ++i) {
        saved[i] = {layers_[i].k_cache, layers_[i].v_cache};
        layers_[i].k_cache = b.k[i] + off;
        layers_[i].v_cache = b.v[i] + off;
    }
    cache_len_ = base;
    cache_cap_ = b.cap;
    auto restore = [&] {
        for (size_t i = 0; i < layers_.size(); ++i) {
            layers_[i].k_cache = saved[i].first;
            layers_[i].v_cache = saved[i].second;
        }
        cache_len_ = saved_len;
        cache_cap_ = saved_cap;
        last_rows_ = saved_rows;
        resident_.resize(std::min(resident_.size(), saved_resident));  // (forward() may have appended the lane's tokens)
    };
    try {
        forward(ids, n);
        hip_check(hipMemcpyAsync(b.logits + (size_t)lane * cfg_.vocab, logits_, (size_t)cfg_.vocab * sizeof(float), hipMemcpyDeviceToDevice, stream_),
                  "D2D logits");
        // (forward left the lane's length in pos_: the single-sequence cache's own length goes back)
        hip_check(hipMemcpyAsync(pos_, &saved_len, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
        hip_check(hipStreamSynchronize(stream_), "sync");
    } catch (...) {
        restore();
        (void)hipMemcpyAsync(pos_, &saved_len, sizeof(int), hipMemcpyHostToDevice, stream_);  // (forward may have left the lane's)
        (void)hipStreamSynchronize(stream_);
        throw;
    }
    restore();
    b.len[lane] = base + n;
}

// The middle of either step body for one layer: the staging rows' Q rotated in place, K rotated (GPT-2: copied) and V copied to
// row pos[lane] of each lane's cache, then the ragged attention (pos[lane] + 1 keys; frozen lanes skipped) and its merge.
void LlmModel::lane_attention(const LaneBank& b, int n, size_t li, float* scratch, float* ctx)
{
    const LlmConfig& c = cfg_;
    const Layer& L = layers_[li];
    const int d = c.head_dim, QD = c.q_dim(), kvh = gpt2_ ? c.heads : c.kv_heads, kv = kvh * d, ldq = QD + 2 * kv;
    const int64_t stride = (int64_t)b.alloc_cap * kv;
    if (c.qwen3())
        hip_check(launch_lane_qk_norm_rope_scatter(b.qkv, ldq, n, c.heads, kvh, d, L.q_norm, L.k_norm, c.eps, cos_, sin_, b.k[li], b.v[li], stride,
                                                   b.cap, b.dev, stream_), "head norm + rotate + scatter");
    else
        hip_check(launch_lane_rope_scatter(b.qkv, ldq, n, c.heads, kvh, d, cos_, sin_, b.k[li], b.v[li], stride, b.cap, b.dev, gpt2_ ? 0 : 1,
                                           stream_), "rotate + scatter");
    hip_check(launch_decode_attention(b.qkv, ldq, n, b.k[li], kv, b.v[li], kv, b.cap, nullptr, b.cap, c.heads, d, -1, splits_, scratch, ctx, QD,
                                      stream_, c.heads / kvh, stride, stride, 1, b.dev.pos, b.dev.live), "attention");
}

// One lock-step step of the lanes bank: pass()'s stages with one row per lane.  Its own first half of the layer -- Q | K | V of
// every lane into the staging rows -- then lane_attention(); embedding, layer_finish, final norm and head are pass()'s.
void LlmModel::lane_step(int n)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const LaneBank& b = lane_bank_;
    const int H = c.hidden, d = c.head_dim, QD = c.q_dim();
    const int kvh = gpt2_ ? c.heads : c.kv_heads, kv = kvh * d, ldq = QD + 2 * kv;
    embed_rows(reinterpret_cast<const uint32_t*>(b.dev.token), n, h_, 0, nullptr, b.dev.pos);
    for (size_t li = 0; li < layers_.size(); ++li) {
        const Layer& L = layers_[li];
        if (fp8_) {
            fp8_qkv(n, L, b.qkv, ldq, b.qkv + QD, b.qkv + QD + kv, ldq, 0, nullptr);
        } else if (quant_) {  // Q | K | V as plain segments into the staging rows (launch_qfused streams the weights once for <= 8 rows)
            QFusedArgs a;
            a.mode = QF_PLAIN;
            quant_source(a, n, h_, H, H, L.ln1, q6(L.q) || q6(L.k) || q6(L.v), "norm + q8k 1");
            a.W[0] = L.q; a.W[1] = L.k; a.W[2] = L.v;
            a.seg_jobs[0] = H / 2; a.seg_jobs[1] = kv / 2; a.seg_jobs[2] = kv / 2;
            a.jobs = H / 2 + kv;
            a.bias = L.bqkv; a.bias_off[1] = H; a.bias_off[2] = H + kv;
            a.Y[0] = b.qkv; a.Y[1] = b.qkv + H; a.Y[2] = b.qkv + H + kv;
            a.ldy[0] = a.ldy[1] = a.ldy[2] = ldq;
            hip_check(launch_qfused(a, s), "norm + qkv");
        } else {
            LlmGemvArgs a;
            a.X = h_; a.ldx = H; a.rows = n; a.gamma = L.ln1; a.beta = L.ln1_b; a.layernorm = gpt2_ ? 1 : 0; a.eps = c.eps; a.W = L.wqkv;
            a.bf16 = bf16_; a.bias = L.bqkv; a.n_out = ldq; a.k = H; a.Y0 = b.qkv; a.ldy0 = ldq;
            project(StepRoute::Lanes, a, "norm + qkv");
        }
        lane_attention(b, n, li, att_scratch_, ctx_);
        layer_finish(StepRoute::Lanes, n, L, false);
    }
    final_norm(h_, n, last_);
    head(StepRoute::Lanes, last_, n, b.logits);
}

void LlmModel::lane_step_enqueue(LaneBank& b, int n)
{
    if (b.wide) wide_step_enqueue(n);
    else lane_step(n);
}

void LlmModel::lane_pick_enqueue(LaneBank& b, int lanes, int first, int advance)
{
    hip_check(launch_lane_pick(b.logits, cfg_.vocab, cfg_.vocab, lanes, first, b.best, b.dev, b.hist, b.hist_stride, b.cap, advance, stream_),
              b.wide ? "wide pick" : "lane pick");
}

void LlmModel::lanes_step(Bank bank, const uint32_t* ids, const int32_t* live, float* hidden_out, float* logits_out)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    LaneBank& b = bank_of(bank);
    if (b.lanes < 1) throw std::runtime_error(b.begin_error);
    const LaneStateRef& h = b.host;
    for (int l = 0; l < b.lanes; ++l) {
        const bool on = live ? live[l] != 0 : true;
        if (on && b.len[l] >= b.cap) throw std::runtime_error("lane " + std::to_string(l) + " is full");
        h.token[l] = (int32_t)ids[l];
        h.pos[l] = b.len[l];
        h.live[l] = on ? 1 : 0;
    }
    lane_state_to_device(b);
    lane_step_enqueue(b, b.lanes);
    hip_check(hipStreamSynchronize(stream_), "sync");
    for (int l = 0; l < b.lanes; ++l)
        if (h.live[l]) b.len[l] += 1;
    const float* hidden = b.wide ? pn_ : last_;  // where the step body's final norm wrote
    if (hidden_out) hip_check(hipMemcpy(hidden_out, hidden, (size_t)b.lanes * cfg_.hidden * sizeof(float), hipMemcpyDeviceToHost), "D2H hidden");
    if (logits_out)
        hip_check(hipMemcpy(logits_out, b.logits, (size_t)b.lanes * cfg_.vocab * sizeof(float), hipMemcpyDeviceToHost), "D2H logits");
}

int LlmModel::lane_cache_len(Bank bank, int lane) const
{
    const LaneBank& b = bank_of(bank);
    if (lane < 0 || lane >= b.lanes) throw std::runtime_error("no such lane");
    return b.len[lane];
}

void LlmModel::lane_kv_rows(Bank bank, int lane, int layer, int first, int rows, float* k_out, float* v_out) const
{
    const LaneBank& b = bank_of(bank);
    if (lane < 0 || lane >= b.lanes) throw std::runtime_error("no such lane");
    if (layer < 0 || layer >= (int)layers_.size() || first < 0 || rows < 0 || first > b.len[lane] || rows > b.len[lane] - first)
        throw std::runtime_error("cache rows out of range");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    const size_t kv = (size_t)(gpt2_ ? cfg_.hidden : cfg_.kv_heads * cfg_.head_dim);
    const size_t off = ((size_t)lane * b.alloc_cap + (size_t)first) * kv, bytes = (size_t)rows * kv * sizeof(float);
    hip_check(hipMemcpy(k_out, b.k[(size_t)layer] + off, bytes, hipMemcpyDeviceToHost), "D2H k cache");
    hip_check(hipMemcpy(v_out, b.v[(size_t)layer] + off, bytes, hipMemcpyDeviceToHost), "D2H v cache");
}

hipGraphExec_t LlmModel::lane_step_graph(LaneBank& b, int n)
{
    if (b.graphs[n]) return b.graphs[n];
    return b.graphs[n] = capture_graph(stream_, [&] {
        lane_step_enqueue(b, n);
        lane_pick_enqueue(b, n, 0, 1);
    });
}

void LlmModel::lane_burst(LaneBank& b, int n, size_t times, hipGraphExec_t chain)
{
    hipGraphExec_t exec = chain ? chain : lane_step_graph(b, n);
    for (size_t i = 0; i < times; ++i) hip_check(hipGraphLaunch(exec, stream_), "graph launch");
    if (!b.wide) return;
    for (const Layer& L : layers_)  // (a replay runs no host code: the routing record's row count of the rows route is set here)
        if (L.moe) L.moe_rec_rows = n;
}

std::vector<std::vector<uint32_t>> LlmModel::generate_lanes(const std::vector<LaneRequest>& reqs, int lanes, int lane_context,
                                                            const std::function<bool(size_t, uint32_t)>& on_token)
{
    if (lanes == 0) lanes = kLanes;
    if (lanes < 1 || lanes > kLanes) throw InvalidConfig("lanes must be 1..8 (0 = 8)");
    return generate_on_lanes(reqs, lanes, lane_context, on_token, lane_bank_, false);
}

std::vector<std::vector<uint32_t>> LlmModel::generate_on_lanes(const std::vector<LaneRequest>& reqs, int lanes, int lane_context,
                                                               const std::function<bool(size_t, uint32_t)>& on_token, LaneBank& b, bool strict)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    auto refuse = [&](const std::string& what) {  // generate_lanes' own refusals keep their types
        if (strict) throw InvalidConfig(what);
        throw std::runtime_error(what);
    };
    bool automata = false;  // some request carries a pattern or a grammar: the constrained chains, the lanes' automaton table
    const int cap = lane_context <= 0 ? cache_cap_ : std::min(cache_cap_, lane_context);
    bool slow = false;  // some request needs its logits row looked at: processors or sampling
    // Log-probabilities: on when some request asks for them and gives a sink; lpk is the width the device computes for every lane
    // (llm.h), each request keeping its own top_k of them.
    bool lp = false;
    int lpk = 1;
    constexpr size_t kSlots = KJARNI_SCORE_TOPK_MAX;
    std::vector<std::vector<uint32_t>> out(reqs.size());
    std::vector<GenerationRun> waiting;  // generate()'s bookkeeping of every request, until a lane takes it
    waiting.reserve(reqs.size());
    for (size_t i = 0; i < reqs.size(); ++i) {  // everything is checked before any GPU work
        const LaneRequest& r = reqs[i];
        if (r.prompt.empty()) refuse("cannot generate from empty prompt (prompt " + std::to_string(i) + ")");
        if ((int64_t)r.prompt.size() > cap)
            throw InvalidConfig("prompt " + std::to_string(i) + " does not fit the lane capacity of " + std::to_string(cap) + " tokens");
        if (r.options.sample && !r.options.uniform) refuse("sampling needs a uniform source (prompt " + std::to_string(i) + ")");
        waiting.emplace_back(r.prompt, r.options, (size_t)cap, cfg_.eos_ids, out[i]);
        if ((int)waiting.back().stops.size() > kMaxLaneStops) refuse("more than 16 stop ids (prompt " + std::to_string(i) + ")");
        if (r.options.constraint || r.options.grammar) {  // generate()'s refusals, by prompt
            const std::string who = " (prompt " + std::to_string(i) + ")";
            if (r.options.constraint && r.options.grammar) throw InvalidConfig("a request takes a constraint or a grammar, not both" + who);
            const int adev = r.options.constraint ? r.options.constraint->device() : r.options.grammar->device();
            const int avocab = r.options.constraint ? r.options.constraint->vocab() : r.options.grammar->vocab();
            const char* what = r.options.constraint ? "constraint" : "grammar";
            if (adev != device_)
                throw InvalidConfig(std::string("the ") + what + " lives on device " + std::to_string(adev) + ", the model on device " +
                                    std::to_string(device_) + who);
            if (avocab != cfg_.vocab)
                throw InvalidConfig(std::string("the ") + what + "'s token table has " + std::to_string(avocab) + " tokens, the model's vocabulary " +
                                    std::to_string(cfg_.vocab) + who);
            try {
                if (r.options.constraint) r.options.constraint->check_states(waiting.back().stops);
                else r.options.grammar->check_states(waiting.back().stops);
            } catch (const InvalidConfig& e) {
                throw InvalidConfig(std::string(e.what()) + who);
            }
            automata = true;
        }
        slow = slow || r.options.sample || r.options.repetition_penalty != 1.0f || r.options.no_repeat_ngram > 0;
        if (r.options.logprobs < -1 || r.options.logprobs > KJARNI_SCORE_TOPK_MAX || r.options.logprobs > cfg_.vocab)
            throw InvalidConfig("top_k (" + std::to_string(r.options.logprobs) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                                "] and not above the vocabulary (" + std::to_string(cfg_.vocab) + ") (prompt " + std::to_string(i) + ")");
        if (r.options.logprobs >= 0 && r.options.logprob_sink) {
            lp = true;
            if (r.options.logprobs > 1) lpk = std::min(KJARNI_SCORE_TOPK_MAX, cfg_.vocab);
        }
    }
    if (reqs.empty()) return out;
    const int n = (int)std::min<size_t>((size_t)lanes, reqs.size());
    ensure_lane_bank(b, n, lane_context);
    if (lp) {
        ensure_logprobs();
        ensure_lane_logprobs(b);
        for (const LaneRequest& r : reqs)
            if (r.options.logprobs >= 0 && r.options.logprob_sink) r.options.logprob_sink->clear(r.options.logprobs);
    }
    if (automata) ensure_lane_automata();
    const LaneLogs& LL = b.logs;
    const LaneStateRef& h = b.host;  // (the mirror's fields)
    auto prefill = [&](int l, int shared, const uint32_t* ids, int count) {  // behind `shared` copied prefix rows
        if (shared >= 1) lane_prefill_shared(b, l, shared, ids, count);
        else lane_prefill_at(b, l, 0, ids, count);
    };
    const size_t vocab = (size_t)cfg_.vocab;
    // Prefix reuse: the prefix every prompt shares (one token short of the shortest prompt, whose last token must be forwarded
    // for its logits) is prefilled once into the single-sequence cache -- where it also stays for the next call -- and copied
    // into each lane that takes a request; the lane prefills the rest behind it.
    // Only the requests that will enter a lane count (generate()'s rule, as start() below applies it: something to generate).
    int shared = 0;
    if (prefix_reuse_) {
        const LaneRequest* head = nullptr;
        size_t lcp = 0;
        for (size_t i = 0; i < reqs.size(); ++i) {
            const LaneRequest& r = reqs[i];
            if (!waiting[i].wants_token()) continue;
            if (!head) {
                head = &r;
                lcp = r.prompt.size() - 1;
                continue;
            }
            lcp = std::min(lcp, r.prompt.size() - 1);
            lcp = prefix_keep_host(head->prompt.data(), head->prompt.size(), r.prompt.data(), r.prompt.size(), lcp);
        }
        shared = (int)lcp;
        if (shared >= 1) {
            const int p = keep_prefix(head->prompt.data(), (size_t)shared, (size_t)shared);
            if (p < shared) forward(head->prompt.data() + p, shared - p);
            else hip_check(hipMemcpyAsync(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
        }
    }

    struct Run {  // the request a lane is working on
        int64_t req = -1;
        size_t seen = 0;
        GenerationRun g;
        std::function<bool(uint32_t)> on_token;  // the caller's, bound to the request
        TokenLogprobs* sink = nullptr;           // where the request's records go (null: it asked for none)
        AutomatonCursor cur;                     // the host's copy of the request's automaton (empty: the request has none)
        ConstraintOutcome outcome;
        ConstraintOutcome* outcome_out = nullptr;
        bool reported = true;                    // the outcome has been written, or there is none to write
    };
    std::vector<Run> run((size_t)n);
    size_t next_req = 0;
    auto take = [&](int l, uint32_t tok) {  // generate()'s drain; true: the token was emitted
        Run& r = run[l];
        if (r.g.done) return false;
        if (!r.cur) return r.g.accept(tok, r.on_token);
        // ... under an automaton, as generate() has it: a stop id ends the request (complete when the state is accepting), any
        // other token moves the host's cursor, and a closed state ends the request behind the token
        if (!r.g.wants_token()) {
            r.g.done = true;
            return false;
        }
        if (r.g.is_stop(tok)) {
            (r.cur.accepting() ? r.outcome.complete : r.outcome.violated) = true;
            r.g.done = true;
            return false;
        }
        if (!r.cur.step(tok)) {
            r.outcome.violated = true;
            r.g.done = true;
            return false;
        }
        const bool taken = r.g.accept(tok, r.on_token);
        if (r.cur.closed()) r.outcome.complete = r.g.done = true;
        return taken;
    };
    // The outcome of the constrained request that lane l has finished: the host's walk, and the lane's row as the device left it
    // (the host's own values where a callback ended the request: the device went on until the host froze the lane).
    auto report = [&](int l) {
        Run& r = run[l];
        if (r.reported) return;
        r.reported = true;
        LaneAutomatonSlot& slot = lane_auto_host_->slot[l];
        hip_check(hipMemcpyAsync(&slot, lane_auto_->slot + l, sizeof(slot), hipMemcpyDeviceToHost, stream_), "D2H lane automaton");
        hip_check(hipStreamSynchronize(stream_), "sync");
        const bool pattern = slot.kind == kLaneKindPattern;
        r.outcome.final_state = r.cur.state();
        r.outcome.final_depth = r.cur.depth();
        r.outcome.accepted = r.cur.accepting();
        r.outcome.violated = r.outcome.violated || (pattern ? slot.crow.violated : slot.grow.violated) != 0;
        r.outcome.device_state = r.g.cancelled ? r.outcome.final_state : pattern ? slot.crow.state : slot.grow.state;
        r.outcome.device_depth = r.g.cancelled ? r.outcome.final_depth : pattern ? 0 : slot.grow.depth;
        if (r.outcome_out) *r.outcome_out = r.outcome;
    };
    auto new_cursor = [](const LaneRequest& q) {
        AutomatonCursor cur;
        cur.con = q.options.constraint;
        cur.gram = q.options.grammar;
        cur.hq = cur.con ? cur.con->dfa().start : 0;
        return cur;
    };
    // the next waiting request that has anything to generate goes into lane l (false: none is left); its prompt is prefilled
    auto start = [&](int l) {
        Run& r = run[l];
        report(l);  // (the request the lane leaves, before its slot is rewritten)
        while (next_req < reqs.size()) {
            const size_t i = next_req++;
            const LaneRequest& q = reqs[i];
            if (!waiting[i].wants_token()) {  // nothing to generate: the automaton stays where it starts
                const AutomatonCursor at = new_cursor(q);
                if (at && q.options.constraint_outcome) {
                    ConstraintOutcome o;
                    o.final_state = o.device_state = at.state();
                    o.accepted = at.accepting();
                    *q.options.constraint_outcome = o;
                }
                continue;
            }
            r.req = (int64_t)i;
            r.seen = 0;
            r.g = std::move(waiting[i]);
            r.on_token = nullptr;
            r.sink = q.options.logprobs >= 0 ? q.options.logprob_sink : nullptr;
            r.cur = new_cursor(q);
            r.outcome = ConstraintOutcome();
            r.outcome_out = q.options.constraint_outcome;
            r.reported = !r.cur;
            if (automata) {  // the lane's slot: the request's view with its own stop ids, and a fresh row
                LaneAutomatonSlot& slot = lane_auto_host_->slot[l];
                std::memset(&slot, 0, sizeof(slot));
                if (r.cur.con) {
                    slot.kind = kLaneKindPattern;
                    slot.cview = r.cur.con->view(r.g.stops);
                    slot.crow.state = r.cur.hq;
                } else if (r.cur.gram) {
                    slot.kind = kLaneKindGrammar;
                    slot.gview = r.cur.gram->view(r.g.stops);
                }
                // (no sync of its own: the stream is in order, the prefill below ends in one, and this host slot is not written
                // again before report() has synchronised)
                hip_check(hipMemcpyAsync(lane_auto_->slot + l, &slot, sizeof(slot), hipMemcpyHostToDevice, stream_), "H2D lane automaton");
            }
            if (on_token) r.on_token = [&on_token, i](uint32_t tok) { return on_token(i, tok); };
            if (shared >= 1) {
                prefill(l, shared, q.prompt.data() + shared, (int)q.prompt.size() - shared);
                prefix_reused_ += (uint64_t)shared;
                prefix_computed_ += q.prompt.size() - (size_t)shared;
            } else {
                prefill(l, 0, q.prompt.data(), (int)q.prompt.size());
                if (prefix_reuse_) prefix_computed_ += q.prompt.size();
            }
            h.token[l] = 0;
            h.pos[l] = (int32_t)q.prompt.size();
            h.live[l] = 1;
            h.count[l] = 0;
            h.limit[l] = (int32_t)r.g.tokens_left();  // the device's copy of the rule: it feeds itself and stops there (LastToken::NotFed)
            h.n_stop[l] = (int32_t)r.g.stops.size();
            for (size_t e = 0; e < r.g.stops.size(); ++e) h.stop[l][e] = (int32_t)r.g.stops[e];
            return true;
        }
        r.req = -1;
        r.g.done = true;
        h.live[l] = 0;
        return false;
    };
    auto any_running = [&] {
        for (int l = 0; l < n; ++l)
            if (!run[l].g.done) return true;
        return false;
    };

    if (!slow) {
        // Greedy without processors: every lane's token, position and live flag stay on the device; one graph replay per step,
        // the host looks every few steps (generate()'s cadence).  Tokens a lane computed past its stop are discarded.
        // a lane's first token comes from its prefill's logits row: the lane pick on that row alone
        auto first_pick = [&](int l) {
            lane_state_to_device(b);
            if (automata) {  // the lane's mask on the prefill's row, the pick, the automaton's first move
                lane_automaton_pick_enqueue(b, l, 1, 0, lp, lpk);
            } else {
                if (lp) lane_logprobs_enqueue(b, l, 1, lpk);  // (the lane's count is 0: record 0 of its new request)
                lane_pick_enqueue(b, 1, l, 0);
            }
            lane_state_from_device(b);
        };
        auto drain = [&](size_t steps) {  // step-major, lane order within a step
            std::vector<std::vector<int32_t>> fresh((size_t)n);
            // the records behind the tokens: the lanes step together, so their new log entries lie in nearly the same columns
            // [lo, hi) of the lanes' logs, and one strided copy per array fetches that window of every lane
            std::vector<size_t> first_new((size_t)n, 0);
            size_t lo = SIZE_MAX, hi = 0;
            for (int l = 0; l < n; ++l) {
                Run& r = run[l];
                const size_t have = (size_t)h.count[l];
                if (r.req < 0 || have <= r.seen) continue;
                const size_t m = have - r.seen, at = (size_t)l * b.hist_stride + r.seen;
                fresh[(size_t)l].resize(m);
                hip_check(hipMemcpyAsync(fresh[(size_t)l].data(), b.hist + at, m * sizeof(int32_t), hipMemcpyDeviceToHost, stream_), "D2H tokens");
                first_new[(size_t)l] = r.seen;
                if (lp && r.sink) {
                    lo = std::min(lo, r.seen);
                    hi = std::max(hi, have);
                }
                r.seen = have;
            }
            const size_t win = hi > lo ? hi - lo : 0;
            std::vector<float> flp((size_t)n * win), ftlp((size_t)n * win * kSlots);
            std::vector<uint32_t> fids((size_t)n * win * kSlots);
            if (win) {
                const size_t pitch = (size_t)b.hist_stride;
                hip_check(hipMemcpy2DAsync(flp.data(), win * sizeof(float), LL.lp + lo, pitch * sizeof(float), win * sizeof(float), (size_t)n,
                                           hipMemcpyDeviceToHost, stream_), "D2H logprobs");
                hip_check(hipMemcpy2DAsync(fids.data(), win * kSlots * sizeof(uint32_t), LL.ids + lo * kSlots, pitch * kSlots * sizeof(uint32_t),
                                           win * kSlots * sizeof(uint32_t), (size_t)n, hipMemcpyDeviceToHost, stream_), "D2H top-k ids");
                hip_check(hipMemcpy2DAsync(ftlp.data(), win * kSlots * sizeof(float), LL.tlp + lo * kSlots, pitch * kSlots * sizeof(float),
                                           win * kSlots * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, stream_), "D2H top-k logprobs");
            }
            hip_check(hipStreamSynchronize(stream_), "sync");
            for (size_t i = 0; i < steps; ++i)
                for (int l = 0; l < n; ++l) {
                    if (i >= fresh[(size_t)l].size()) continue;
                    Run& r = run[l];
                    if (take(l, (uint32_t)fresh[(size_t)l][i]) && lp && r.sink) {
                        const size_t at = (size_t)l * win + (first_new[(size_t)l] + i - lo);  // the token's log entry in the window
                        r.sink->push(flp[at], fids.data() + at * kSlots, ftlp.data() + at * kSlots);
                    }
                }
        };
        const size_t burst = on_token ? 4 : 16;
        for (;;) {
            // a lane that has no request, or whose request ended (on the device, or by the host's rules: a callback said stop),
            // takes the next waiting one; its first token comes from the prefill's row
            bool dirty = false;
            for (int l = 0; l < n; ++l) {
                Run& r = run[l];
                if (!r.g.done && !h.live[l]) r.g.done = true;
                if (r.g.done && h.live[l]) {
                    h.live[l] = 0;
                    dirty = true;
                }
                while (r.g.done && next_req < reqs.size()) {
                    if (!start(l)) break;
                    first_pick(l);  // (writes the whole state, this pass's edits included)
                    dirty = false;
                    b.len[l] = h.pos[l];
                    drain(1);
                    if (!h.live[l]) r.g.done = true;
                }
            }
            if (!any_running()) break;
            if (dirty) lane_state_to_device(b);
            // (with records: the chain that has them in it, captured per (bank, lanes, width))
            // (under automata: the chain with the lane apply and advance around the pick, one per (bank, lanes, records))
            lane_burst(b, n, burst, automata ? lane_automaton_step_graph(b, n, lp, lpk) : lp ? lane_logprob_step_graph(b, n, lpk) : nullptr);
            lane_state_from_device(b);
            for (int l = 0; l < n; ++l)
                if (run[l].req >= 0) b.len[l] = h.pos[l];
            drain(burst);
        }
        for (int l = 0; l < n; ++l) report(l);
        return out;
    }

    // Processors / sampling: every lane's next token is decided from that lane's logits row -- the processors on the device
    // with the lane's own history and counts (launch_logits_processors), then the device argmax (four bytes back) or, for a
    // sampled request, the row to the host and generate()'s full-array sampler with the request's own uniform source.  The
    // step itself is the same chain of launches, enqueued directly (no graph): correct first, fast later.
    ensure_host_logits();
    std::vector<float> probs;
    std::vector<uint32_t> ids;
    auto pstate = [&](int l, int32_t*& tok, int32_t*& distinct, int*& counts, int*& nd) {
        tok = b.ptok + (size_t)l * b.hist_stride;
        distinct = b.pdistinct + (size_t)l * b.hist_stride;
        counts = b.pcounts + (size_t)l * vocab;
        nd = b.pndistinct + l;
    };
    auto begin_history = [&](int l) {  // the history so far = the prompt
        const Run& r = run[l];
        int32_t *tok, *distinct;
        int *counts, *nd;
        pstate(l, tok, distinct, counts, nd);
        begin_token_history(tok, r.g.all.data(), r.g.all.size(), counts, distinct, nd);
        hip_check(hipStreamSynchronize(stream_), "sync");
    };
    for (int l = 0; l < n; ++l)
        if (start(l)) begin_history(l);
    while (any_running()) {
        for (int l = 0; l < n; ++l) {  // decide, in lane order
            Run& r = run[l];
            // (a lane whose request ends takes the next one and decides its first token in the same round, from the prefill's row:
            // the round's step rewrites every row)
            while (!r.g.done) {
                const GenerateOptions& o = reqs[(size_t)r.req].options;
                float* row = b.logits + (size_t)l * vocab;
                int32_t *tok, *distinct;
                int *counts, *nd;
                pstate(l, tok, distinct, counts, nd);
                const bool rec = lp && r.sink, edits = o.repetition_penalty != 1.0f || o.no_repeat_ngram > 0 || r.cur;
                if (rec) logprob_partial_on(row, 1, nullptr, lpk, LL.scratch, edits ? LL.copy : nullptr);  // ahead of the mask and the processors
                // the lane's mask, through the single-row launchers on the lane's slot of the table
                if (r.cur.con)
                    hip_check(launch_constraint_apply(row, (int64_t)vocab, 1, (int)vocab, &lane_auto_->slot[l].cview, &lane_auto_->slot[l].crow, stream_),
                              "constraint apply");
                if (r.cur.gram)
                    hip_check(launch_grammar_apply(row, (int64_t)vocab, 1, (int)vocab, &lane_auto_->slot[l].gview, &lane_auto_->slot[l].grow, stream_),
                              "grammar apply");
                if (o.repetition_penalty != 1.0f || o.no_repeat_ngram > 0)
                    hip_check(launch_logits_processors(row, (int)vocab, tok, (int)r.g.all.size(), counts, distinct, nd, o.repetition_penalty,
                                                       o.no_repeat_ngram, stream_), "logits processors");
                uint32_t next;
                if (o.sample) {
                    hip_check(hipMemcpyAsync(host_logits_, row, vocab * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H logits");
                    hip_check(hipStreamSynchronize(stream_), "sync");
                    sampling_distribution(host_logits_, vocab, o.sampling, ids, probs);
                    next = sample_from_distribution(ids, probs, o.uniform(), vocab);
                    ++tokens_from_logits_;
                } else {
                    hip_check(launch_argmax(row, (int)vocab, best_, token_, nullptr, nullptr, nullptr, stream_), "argmax");
                    int32_t t = 0;
                    hip_check(hipMemcpyAsync(&t, token_, sizeof(t), hipMemcpyDeviceToHost, stream_), "D2H token");
                    hip_check(hipStreamSynchronize(stream_), "sync");
                    next = (uint32_t)t;
                    ++tokens_from_candidates_;
                }
                const bool taken = take(l, next);
                if (taken && rec) {  // the record at the token's index in the request's output, in the lane's own log
                    hip_check(hipMemsetD32Async((hipDeviceptr_t)lp_tok_, (int)next, 1, stream_), "token");
                    logprob_finish_on(row, 1, nullptr, lpk, LL.scratch, edits ? LL.copy : row, lp_tok_, nullptr, (int)r.g.out->size() - 1, LL.stride,
                                      LL.lp + (size_t)l * LL.stride, LL.ids + (size_t)l * LL.stride * kSlots,
                                      LL.tlp + (size_t)l * LL.stride * kSlots);
                }
                if (taken && r.cur) {  // the device's automaton takes the host's choice (fed or not, so that it ends where the host's does)
                    hip_check(hipMemsetD32Async((hipDeviceptr_t)token_, (int)next, 1, stream_), "token");
                    if (r.cur.con)
                        hip_check(launch_constraint_advance(token_, 1, &lane_auto_->slot[l].cview, &lane_auto_->slot[l].crow, nullptr, nullptr, 0, stream_),
                                  "constraint advance");
                    else
                        hip_check(launch_grammar_advance(token_, 1, &lane_auto_->slot[l].gview, &lane_auto_->slot[l].grow, nullptr, nullptr, nullptr, 0,
                                                         stream_), "grammar advance");
                }
                // LastToken::NotFed: a request that has its max_new_tokens leaves the lane at once (asked whatever take() did:
                // a refused token leaves the run done, which answers no)
                if (!r.g.feeds_accepted(LastToken::NotFed)) r.g.done = true;
                if (!r.g.done) {  // the token is the lane's next input, at the position it took in the sequence
                    h.token[l] = (int32_t)next;
                    h.pos[l] = (int32_t)r.g.all.size() - 1;
                    h.live[l] = 1;
                    int32_t* slot = tok + (r.g.all.size() - 1);
                    hip_check(hipMemcpyAsync(slot, &h.token[l], sizeof(int32_t), hipMemcpyHostToDevice, stream_), "H2D history");
                    hip_check(launch_token_counts(slot, 1, (int)vocab, counts, distinct, nd, stream_), "token counts");
                    hip_check(hipStreamSynchronize(stream_), "sync");
                    break;
                }
                h.live[l] = 0;
                if (rec && !r.g.out->empty()) {  // the request has ended: its records, before the lane's log starts over
                    const size_t m = r.g.out->size(), at = (size_t)l * LL.stride;
                    std::vector<float> flp(m), ftlp(m * kSlots);
                    std::vector<uint32_t> fids(m * kSlots);
                    hip_check(hipMemcpyAsync(flp.data(), LL.lp + at, m * sizeof(float), hipMemcpyDeviceToHost, stream_), "D2H logprobs");
                    hip_check(hipMemcpyAsync(fids.data(), LL.ids + at * kSlots, m * kSlots * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_),
                              "D2H top-k ids");
                    hip_check(hipMemcpyAsync(ftlp.data(), LL.tlp + at * kSlots, m * kSlots * sizeof(float), hipMemcpyDeviceToHost, stream_),
                              "D2H top-k logprobs");
                    hip_check(hipStreamSynchronize(stream_), "sync");
                    for (size_t i = 0; i < m; ++i) r.sink->push(flp[i], fids.data() + i * kSlots, ftlp.data() + i * kSlots);
                }
                if (start(l)) begin_history(l);
            }
        }
        bool step = false;
        for (int l = 0; l < n; ++l) step = step || h.live[l];
        if (step) {
            lane_state_to_device(b);
            lane_step_enqueue(b, n);
            hip_check(hipStreamSynchronize(stream_), "sync");
            for (int l = 0; l < n; ++l)
                if (h.live[l]) b.len[l] = h.pos[l] + 1;
        }
    }
    for (int l = 0; l < n; ++l) report(l);
    return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// Wide lanes: 9..64 sequences in lock step.  The lanes' state, staging layout, scatter, ragged attention and pick, with every
// projection on the prompt GEMM (one 64-row M-tile: the weights are read once per step whatever the width) instead of the
// 8-row GEMV kernels.  The scheduling loop is generate_on_lanes() above, on the wide bank.

void LlmModel::set_fp8_matrix_cores(bool on)
{
    if (!fp8_ || on == fp8_mc_) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(stream_), "sync");
    drop_lane_graphs(wide_bank_);  // (they hold the route's launches)
    wide_bank_.lanes = 0;       // a wide session ends here: lanes_begin() decides again
    fp8_mc_ = on;
}

// One wide step, a linear chain on the model's stream: the embedding at the lanes' positions, per layer norm 1 -> ONE GEMM of
// the fused [Q;K;V] matrix into the lanes' staging rows -> rotate-and-scatter -> ragged attention -> rows_finish() (o-proj,
// norm 2, SwiGLU / GPT-2 MLP / the MoE rows hook), then the final norm and the head as a GEMM into the bank's logits.  Frozen lanes
// ride along as rows of the GEMMs (each output row depends on its own input row only); the scatter and the attention skip them.
void LlmModel::wide_step_enqueue(int n)
{
    hipStream_t s = stream_;
    const LlmConfig& c = cfg_;
    const int H = c.hidden, d = c.head_dim, QD = c.q_dim();
    const int kvh = gpt2_ ? c.heads : c.kv_heads, kv = kvh * d, ldq = QD + 2 * kv;
    const LaneBank& b = wide_bank_;
    embed_rows(reinterpret_cast<const uint32_t*>(b.dev.token), n, ph_, 0, nullptr, b.dev.pos);
    for (size_t li = 0; li < layers_.size(); ++li) {
        const Layer& L = layers_[li];
        if (gpt2_) hip_check(launch_layernorm(ph_, L.ln1, L.ln1_b, c.eps, n, H, pn_, s), "ln_1");
        else hip_check(launch_rmsnorm(ph_, L.ln1, c.eps, n, H, pn_, s), "rmsnorm 1");
        if (fp8_) {  // three matrices of their own (ensure_lane_bank: only with the switch on), each into its column segment of the rows
            prompt_proj(n, pn_, H, nullptr, L.bqkv, nullptr, b.qkv, ldq, QD, H, nullptr, "q proj", nullptr, false, &L.fq);
            prompt_proj(n, pn_, H, nullptr, L.bqkv ? L.bqkv + QD : nullptr, nullptr, b.qkv + QD, ldq, kv, H, nullptr, "k proj", nullptr, false,
                        &L.fk);
            prompt_proj(n, pn_, H, nullptr, L.bqkv ? L.bqkv + QD + kv : nullptr, nullptr, b.qkv + QD + kv, ldq, kv, H, nullptr, "v proj", nullptr,
                        false, &L.fv);
        } else {
            prompt_proj(n, pn_, H, L.wqkv, L.bqkv, nullptr, b.qkv, ldq, ldq, H, nullptr, "q|k|v proj");
        }
        lane_attention(b, n, li, b.att, pctx_);
        rows_finish(n, L);
    }
    final_norm(ph_, n, pn_);  // (the norm buffer is free behind the last layer)
    prompt_proj(n, pn_, H, lm_head_, nullptr, nullptr, b.logits, c.vocab, c.vocab, H, nullptr, "lm head");
}

std::vector<std::vector<uint32_t>> LlmModel::generate_wide(const std::vector<LaneRequest>& reqs, int lanes, int lane_context,
                                                           const std::function<bool(size_t, uint32_t)>& on_token)
{
    if (lanes < 0 || lanes > kWideLanes) throw InvalidConfig("lanes must be 0..64 (0 = 64)");
    if (lanes == 0) lanes = kWideLanes;
    const size_t width = std::min<size_t>((size_t)lanes, reqs.size());
    if (width <= (size_t)kLanes)  // generate_lanes' route (its GEMV step), under this entry's refusals
        return generate_on_lanes(reqs, (int)std::max<size_t>(width, 1), lane_context, on_token, lane_bank_, true);
    return generate_on_lanes(reqs, lanes, lane_context, on_token, wide_bank_, true);
}

// ---------------------------------------------------------------------------------------------------------------------
// Prompt-lookup decoding: greedy generation that emits several tokens per step.  The draft of a step is the continuation of
// the latest longest n-gram match of the history's suffix in the history itself (no second model); the verify step runs the
// last token and the draft as one causal block of rows at the device-held position and the pick keeps the model's own argmax
// tokens up to and including the first that differs from the draft.  draft -> step -> pick is one linear chain of launches
// on one stream: 1 + (the step's) + 2 launches, captured once per row count.

void check_lookup_config(const LookupConfig& c)
{
    if (c.draft_tokens < 1 || c.draft_tokens > kLookupMaxDraft) throw InvalidConfig("draft_tokens must be 1..7");
    if (c.ngram_max < 1 || c.ngram_max > kLookupMaxNgram) throw InvalidConfig("ngram_max must be 1..4");
    if (c.ngram_min < 1 || c.ngram_min > c.ngram_max) throw InvalidConfig("ngram_min must be 1..ngram_max");
}

// The rule lookup_draft_kernel computes, position by position: the largest (match length, continuation length, position).
std::vector<uint32_t> lookup_draft_host(const uint32_t* T, size_t n, const LookupConfig& c)
{
    size_t best_m = 0, best_c = 0, best_e = 0;
    for (size_t e = 1; e < n; ++e) {
        size_t m = 0;
        while (m < (size_t)c.ngram_max && m < e && T[e - 1 - m] == T[n - 1 - m]) ++m;
        if (m < (size_t)c.ngram_min) continue;
        const size_t cont = std::min((size_t)c.draft_tokens, n - e);
        if (m > best_m || (m == best_m && cont >= best_c)) {  // (e grows: on equal (m, cont) the later position wins)
            best_m = m;
            best_c = cont;
            best_e = e;
        }
    }
    return best_m ? std::vector<uint32_t>(T + best_e, T + best_e + best_c) : std::vector<uint32_t>();
}

void LlmModel::ensure_lookup()
{
    if (vlogits_) return;
    lk_hist_cap_ = cache_cap_ + 16;
    vids_ = reinterpret_cast<uint32_t*>(dalloc(kLanes));
    lk_state_ = reinterpret_cast<LlmLookupState*>(dalloc((sizeof(LlmLookupState) + 3) / 4));
    lk_hist_ = reinterpret_cast<int32_t*>(dalloc((size_t)lk_hist_cap_));
    lk_log_ = reinterpret_cast<int32_t*>(dalloc(2 * (size_t)lk_hist_cap_));
    lk_best_ = reinterpret_cast<unsigned long long*>(dalloc(2 * kLanes));
    hip_check(hipMemset(lk_best_, 0, sizeof(unsigned long long) * kLanes), "memset");
    hip_check(hipMemset(lk_state_, 0, sizeof(LlmLookupState)), "memset");
    vlogits_ = dalloc((size_t)kLanes * cfg_.vocab);
}

LlmModel::StreamScope::StreamScope(LlmModel* model, hipStream_t stream) : model_(model), saved_(nullptr)
{
    if (!model_) return;
    hip_check(hipStreamSynchronize(model_->stream_), "sync");  // what the model enqueued on its own stream is done
    saved_ = model_->stream_;
    model_->stream_ = stream;
}

LlmModel::StreamScope::~StreamScope()
{
    if (model_) model_->stream_ = saved_;
}

// The draft of a verify step, enqueued on stream_.  The lookup rule: one launch.  A drafter (which enqueues on stream_ too: the
// caller holds a StreamScope and has called ensure_lookup() on it): begin, one 2-row pass at n - 2, then rows - 2 single-row
// steps that each read the id handed over before them; rows == 1: the begin alone, no drafter kernel.  The 2-row pass takes the
// verify route (the multi-row weight-streaming kernels, both rows' logits in the drafter's vlogits_, of which row 1 is used):
// measured on the Llama-1B shape it costs 0.93 ms there against 1.42 ms on the non-verify route, whose projections of 2 .. 8
// rows are the prompt's one-wave-per-column kernels (a plain step: 0.62 ms).
void LlmModel::enqueue_draft(int rows, const DraftSource& src)
{
    if (!src.drafter) {
        hip_check(launch_lookup_draft(lk_hist_, lk_state_, src.ngram_max, src.ngram_min, rows - 1, rows, vids_, stream_), "lookup draft");
        return;
    }
    LlmModel& d = *src.drafter;
    hip_check(launch_draft_begin(lk_hist_, lk_hist_cap_, lk_state_, rows, d.ids_, d.pos_, vids_, stream_), "draft begin");
    if (rows < 2) return;
    d.pass(d.ids_, 2, true, true);
    hip_check(launch_draft_handoff(d.vlogits_ + d.cfg_.vocab, d.cfg_.vocab, d.best_, vids_ + 1, d.pos_, 2, stream_), "draft hand-off");
    for (int i = 1; i <= rows - 2; ++i) {
        d.pass(vids_ + i, 1, true);
        hip_check(launch_draft_handoff(d.logits_, d.cfg_.vocab, d.best_, vids_ + i + 1, d.pos_, 1, stream_), "draft hand-off");
    }
}

void LlmModel::enqueue_verify(int rows, const DraftSource* src, bool record)
{
    if (src) enqueue_draft(rows, *src);
    pass(vids_, rows, true, true);
    hip_check(launch_lookup_pick(vlogits_, cfg_.vocab, cfg_.vocab, rows, vids_, lk_best_, lk_state_, record ? lk_hist_ : nullptr, lk_hist_cap_,
                                 pos_, record ? lk_log_ : nullptr, lk_hist_cap_, stream_), "lookup pick");
}

hipGraphExec_t LlmModel::lookup_graph(int rows, const DraftSource& c)
{
    // (arguments of the captured draft launch, or the drafter whose pointers the captured chain holds)
    if (lookup_ngram_[0] != c.ngram_max || lookup_ngram_[1] != c.ngram_min || lookup_serial_ != c.serial()) {
        hip_check(hipStreamSynchronize(stream_), "sync");
        drop_graphs(lookup_graphs_);
        lookup_ngram_[0] = c.ngram_max;
        lookup_ngram_[1] = c.ngram_min;
        lookup_serial_ = c.serial();
    }
    if (lookup_graphs_[rows]) return lookup_graphs_[rows];
    return lookup_graphs_[rows] = capture_graph(stream_, [&] { enqueue_verify(rows, &c, true); });
}

// The ids of a verify block: the token, the draft, and the draft's last id again in the rows past it.
static void verify_block_ids(uint32_t token, const uint32_t* draft, int n_draft, int rows, uint32_t* ids)
{
    ids[0] = token;
    for (int r = 1; r < rows; ++r) ids[r] = r <= n_draft ? draft[r - 1] : ids[r - 1];
}

int LlmModel::verify_step(uint32_t token, const uint32_t* draft, int n_draft, int rows, uint32_t* tokens_out, float* logits_out)
{
    if (n_draft < 0 || n_draft > kLookupMaxDraft) throw InvalidConfig("n_draft must be 0..7");
    if (rows < n_draft + 1 || rows > kLanes) throw InvalidConfig("rows must be n_draft + 1 .. 8");
    if (cache_len_ + rows > cache_cap_)
        throw InvalidConfig("cache_len + rows (" + std::to_string(cache_len_) + " + " + std::to_string(rows) + ") exceeds the context of " +
                            std::to_string(cache_cap_) + " tokens");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ensure_lookup();
    uint32_t ids[kLanes];
    verify_block_ids(token, draft, n_draft, rows, ids);
    LlmLookupState st = {};
    st.n = cache_len_ + 1;
    st.m = n_draft;
    hip_check(hipMemcpyAsync(vids_, ids, sizeof(uint32_t) * (size_t)rows, hipMemcpyHostToDevice, stream_), "H2D ids");
    hip_check(hipMemcpyAsync(lk_state_, &st, sizeof(st), hipMemcpyHostToDevice, stream_), "H2D lookup state");
    hip_check(hipMemcpyAsync(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    enqueue_verify(rows, nullptr, false);
    hip_check(hipMemcpyAsync(&st, lk_state_, sizeof(st), hipMemcpyDeviceToHost, stream_), "D2H lookup state");
    hip_check(hipStreamSynchronize(stream_), "sync");
    for (int i = 0; i <= st.a; ++i) tokens_out[i] = (uint32_t)st.picks[i];
    cache_len_ += st.a + 1;
    last_rows_ = rows;
    if (logits_out)
        hip_check(hipMemcpy(logits_out, vlogits_, (size_t)(n_draft + 1) * cfg_.vocab * sizeof(float), hipMemcpyDeviceToHost), "D2H logits");
    return st.a;
}

std::vector<uint32_t> LlmModel::generate_lookup(const std::vector<uint32_t>& prompt, const GenerateOptions& opt, const LookupConfig& lk,
                                                const std::function<bool(uint32_t)>& on_token, LookupStats* stats)
{
    if (stats) *stats = LookupStats();
    check_lookup_config(lk);
    if (opt.constraint) throw InvalidConfig("generate_lookup does not take a constraint (generate does)");
    if (opt.grammar) throw InvalidConfig("generate_lookup does not take a grammar (generate does)");
    if (opt.sample || opt.repetition_penalty != 1.0f || opt.no_repeat_ngram > 0 || opt.logprobs >= 0)
        return generate(prompt, opt, on_token);  // not applicable (log-probabilities: the plain loop records them)
    DraftSource src;
    src.ngram_max = lk.ngram_max;
    src.ngram_min = lk.ngram_min;
    return greedy_draft_loop(prompt, opt, src, lk.draft_tokens, on_token, stats);
}

// The drafter's side of a loop's start: its own stream is synchronised, its cache holds the prompt (by its own prefix-reuse
// switch).  The caller then holds a StreamScope for the rounds.
void LlmModel::drafter_begin(const DraftSource& src, const std::vector<uint32_t>& prompt)
{
    if (!src.drafter) return;
    hip_check(hipStreamSynchronize(src.drafter->stream_), "sync");
    src.drafter->ensure_lookup();  // (the rows of its 2-row pass land in its vlogits_: allocated here, never inside a capture)
    src.drafter->begin_sequence(prompt);
}

// ... and of its end.  A round on a history of n tokens leaves valid drafter rows for T[0 .. n - 2 + min(a, m - 1)]: with the
// target's cache at cache_len_ rows, rows [0, cache_len_ - 1) of the drafter hold the target's tokens whatever was accepted.
void LlmModel::drafter_leave(const DraftSource& src, const std::vector<uint32_t>& all, bool rounds_ran)
{
    if (!src.drafter || !rounds_ran) return;  // (no round: the drafter is as begin_sequence(prompt) left it)
    LlmModel& d = *src.drafter;
    d.cache_len_ = cache_len_ - 1;
    d.last_rows_ = 1;
    d.resident_.assign(all.begin(), all.begin() + (ptrdiff_t)std::min(all.size(), (size_t)d.cache_len_));
    hip_check(hipMemcpyAsync(d.pos_, &d.cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    hip_check(hipStreamSynchronize(stream_), "sync");
}

std::vector<uint32_t> LlmModel::greedy_draft_loop(const std::vector<uint32_t>& prompt, const GenerateOptions& opt, const DraftSource& src,
                                                  int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats)
{
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (prompt.empty()) throw std::runtime_error("cannot generate from empty prompt");
    if ((int)prompt.size() > cache_cap_) throw InvalidConfig("prompt does not fit the context");
    ensure_lookup();
    begin_sequence(prompt);
    drafter_begin(src, prompt);
    StreamScope on_this_stream(src.drafter, stream_);
    bool rounds_ran = false;
    std::vector<uint32_t> out;
    GenerationRun run(prompt, opt, (size_t)cache_cap_, cfg_.eos_ids, out);
    const std::vector<uint32_t>& all = run.all;
    if (run.done) return out;  // (resident_ = the prompt, from begin_sequence)
    // the first pick comes from the prompt's logits; the history on the device = the prompt + that pick
    run.accept(argmax(), on_token);
    if (run.done) return out;
    LlmLookupState st = {};
    st.n = (int32_t)all.size();
    hip_check(hipMemcpyAsync(lk_hist_, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_), "H2D history");
    hip_check(hipMemcpyAsync(lk_state_, &st, sizeof(st), hipMemcpyHostToDevice, stream_), "H2D lookup state");
    hip_check(hipStreamSynchronize(stream_), "sync");  // (`all` grows below: the copy must have read it)
    const size_t burst = on_token ? 4 : 16;
    std::vector<int32_t> toks(burst * kLanes), log(2 * burst);
    int known_n = st.n, known_steps = 0;
    // The device feeds itself (the verify step's pick is the next step's input), a burst at a time: what it leaves in the cache is
    // where its history stands, all.size() - 1 or further (picks past the end of the run).
    while (!run.done) {
        // a step of `rows` rows writes cache rows [pos, pos + rows) and moves pos by at most `rows`: `steps` of them stay inside
        // the cache whatever they accept while cache_len_ + steps * rows <= capacity; near the end the steps get narrower
        const int room = cache_cap_ - cache_len_;
        if (room <= 0) break;
        const int rows = std::min(draft_tokens + 1, room);
        const size_t steps = std::min(std::min(burst, (size_t)(room / rows)), run.max_new - out.size());
        hipGraphExec_t exec = lookup_graph(rows, src);
        for (size_t i = 0; i < steps; ++i) hip_check(hipGraphLaunch(exec, stream_), "graph launch");
        rounds_ran = rounds_ran || steps > 0;
        hip_check(hipMemcpyAsync(&st, lk_state_, sizeof(st), hipMemcpyDeviceToHost, stream_), "D2H lookup state");
        hip_check(hipMemcpyAsync(toks.data(), lk_hist_ + known_n, steps * (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, stream_),
                  "D2H tokens");
        hip_check(hipMemcpyAsync(log.data(), lk_log_ + 2 * (size_t)known_steps, 2 * steps * sizeof(int32_t), hipMemcpyDeviceToHost, stream_),
                  "D2H step log");
        hip_check(hipStreamSynchronize(stream_), "sync");
        size_t off = 0;
        for (size_t i = 0; i < steps; ++i) {  // in order; tokens past the end are discarded
            const int m = log[2 * i], a = log[2 * i + 1];
            if (!run.done) {
                if (stats) stats->count(rows, m, a);
                for (int j = 0; j <= a && !run.done; ++j) run.accept((uint32_t)toks[off + (size_t)j], on_token);
            }
            off += (size_t)a + 1;
        }
        known_n = st.n;
        known_steps = st.steps;
        cache_len_ = st.n - 1;
    }
    leave_resident(all);  // (`all` is a prefix of the device history: rows of rejected drafts and of picks past the end do not count)
    drafter_leave(src, all, rounds_ran);
    return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// Prompt-lookup decoding for sampled requests (llm.h).  The device side of a step: draft -> verify pass -> rows penalty -> rows
// cut, captured once per row count; the copy of [8 headers | the first 512 candidates of each row] follows the replay.

void LlmModel::ensure_lookup_sampled()
{
    ensure_lookup();
    ensure_sampling();
    ensure_host_logits();
    if (ls_scratch_) return;
    const size_t out_bytes = (size_t)kLanes * sizeof(SampleHeader) + sample_rows_entries(kRowsCandCap) * sizeof(SampleCandidate);
    ls_scratch_ = dalloc((sample_scratch_rows_bytes(kLanes) + 3) / 4);
    hip_check(hipMemset(ls_scratch_, 0, sample_scratch_rows_bytes(kLanes)), "memset");
    ls_out_ = reinterpret_cast<uint8_t*>(dalloc(out_bytes / 4));
    hip_check(hipMemset(ls_out_, 0, out_bytes), "memset");
    ls_up_ = reinterpret_cast<int32_t*>(dalloc(16));
    hip_check(hipHostMalloc((void**)&ls_host_, out_bytes + 32 * sizeof(int32_t), hipHostMallocDefault), "hipHostMalloc");
    ls_up_host_ = reinterpret_cast<int32_t*>(ls_host_ + out_bytes);
    ls_draft_host_ = reinterpret_cast<uint32_t*>(ls_up_host_ + 16);
}

void LlmModel::rows_cut(float* logits, int rows, const GenerateOptions& opt)
{
    const int vocab = cfg_.vocab;
    SampleHeader* headers = reinterpret_cast<SampleHeader*>(ls_out_);
    SampleCandidate* cands = reinterpret_cast<SampleCandidate*>(ls_out_ + kLanes * sizeof(SampleHeader));
    if (opt.repetition_penalty != 1.0f)
        hip_check(launch_repetition_penalty_rows(logits, vocab, rows, vocab, vids_, samp_counts_, samp_distinct_, samp_ndistinct_,
                                                 opt.repetition_penalty, stream_), "rows penalty");
    hip_check(launch_sample_candidates_rows(logits, vocab, rows, vocab, opt.sampling.top_k, opt.sampling.top_p, opt.sampling.min_p, ls_scratch_,
                                            headers, cands, kRowsCandCap, stream_), "rows cut");
}

void LlmModel::enqueue_verify_sampled(int rows, const DraftSource* src, const GenerateOptions& opt)
{
    if (src) enqueue_draft(rows, *src);
    pass(vids_, rows, true, true);
    rows_cut(vlogits_, rows, opt);
}

hipGraphExec_t LlmModel::lookup_sampled_graph(int rows, const DraftSource& c, const GenerateOptions& opt)
{
    LookupSampledArgs want;
    want.ngram_max = c.ngram_max; want.ngram_min = c.ngram_min; want.serial = c.serial();
    want.top_k = opt.sampling.top_k; want.top_p = opt.sampling.top_p; want.min_p = opt.sampling.min_p; want.penalty = opt.repetition_penalty;
    const auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; };  // (bitwise: a NaN equals itself)
    if (want.ngram_max != ls_args_.ngram_max || want.ngram_min != ls_args_.ngram_min || want.serial != ls_args_.serial ||
        want.top_k != ls_args_.top_k ||
        !same(want.top_p, ls_args_.top_p) || !same(want.min_p, ls_args_.min_p) ||
        !same(want.penalty, ls_args_.penalty)) {  // (arguments of the captured launches)
        hip_check(hipStreamSynchronize(stream_), "sync");
        drop_graphs(lookup_sampled_graphs_);
        ls_args_ = want;
    }
    if (lookup_sampled_graphs_[rows]) return lookup_sampled_graphs_[rows];
    return lookup_sampled_graphs_[rows] = capture_graph(stream_, [&] { enqueue_verify_sampled(rows, &c, opt); });
}

// One row's token from what the step's copy brought over (header + candidates of `row` in the pinned mirror); the row's
// processed logits are fetched only when the candidates decline.
uint32_t LlmModel::decide_row(const float* logits_dev, int row, const GenerateOptions& opt, float uniform)
{
    const SampleHeader* headers = reinterpret_cast<const SampleHeader*>(ls_host_);
    const size_t cand_off = kLanes * sizeof(SampleHeader);
    const SampleCandidate* cand = reinterpret_cast<const SampleCandidate*>(ls_host_ + cand_off);
    return sample_row(device_sampling_ ? headers + row : nullptr, kSampleRowsChunk, kRowsCandCap,
                      [&](size_t i) -> const SampleCandidate& { return cand[sample_rows_slot(row, (int)i)]; },
                      [&](size_t n) {  // the later chunks of this row
                          for (size_t s0 = kSampleRowsChunk; s0 < n; s0 += kSampleRowsChunk) {
                              const size_t at = cand_off + sample_rows_slot(row, (int)s0) * sizeof(SampleCandidate);
                              hip_check(hipMemcpyAsync(ls_host_ + at, ls_out_ + at, std::min<size_t>(kSampleRowsChunk, n - s0) * sizeof(SampleCandidate),
                                                       hipMemcpyDeviceToHost, stream_), "D2H candidates");
                          }
                          hip_check(hipStreamSynchronize(stream_), "sync");
                      },
                      logits_dev + (size_t)row * (size_t)cfg_.vocab, opt.sampling, uniform, nullptr);  // (the penalty already ran, on the device)
}

int LlmModel::verify_step_sampled(uint32_t token, const uint32_t* draft, int n_draft, int rows, const GenerateOptions& opt,
                                  const uint32_t* history, size_t n_history, const float* uniforms, uint32_t* picks_out,
                                  int* draws_used, float* logits_out)
{
    if (n_draft < 0 || n_draft > kLookupMaxDraft) throw InvalidConfig("n_draft must be 0..7");
    if (rows < n_draft + 1 || rows > kLanes) throw InvalidConfig("rows must be n_draft + 1 .. 8");
    if (!opt.sample) throw InvalidConfig("verify_step_sampled needs a sampling request");
    if (opt.no_repeat_ngram > 0) throw InvalidConfig("the n-gram ban is not built for verify rows");
    if (cache_len_ + rows > cache_cap_)
        throw InvalidConfig("cache_len + rows (" + std::to_string(cache_len_) + " + " + std::to_string(rows) + ") exceeds the context of " +
                            std::to_string(cache_cap_) + " tokens");
    const bool penalty = opt.repetition_penalty != 1.0f;
    if (penalty && (!history || n_history == 0 || history[n_history - 1] != token || n_history > (size_t)cache_cap_ + 1))
        throw InvalidConfig("history must end with the token and hold at most context + 1 tokens");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ensure_lookup_sampled();
    const int vocab = cfg_.vocab;
    uint32_t ids[kLanes];
    verify_block_ids(token, draft, n_draft, rows, ids);
    hip_check(hipMemcpyAsync(vids_, ids, sizeof(uint32_t) * (size_t)rows, hipMemcpyHostToDevice, stream_), "H2D ids");
    hip_check(hipMemcpyAsync(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    if (penalty) begin_token_history(samp_tokens_, history, n_history, samp_counts_, samp_distinct_, samp_ndistinct_);
    enqueue_verify_sampled(rows, nullptr, opt);
    const size_t bytes = kLanes * sizeof(SampleHeader) + (size_t)rows * kSampleRowsChunk * sizeof(SampleCandidate);
    hip_check(hipMemcpyAsync(ls_host_, ls_out_, bytes, hipMemcpyDeviceToHost, stream_), "D2H candidates");
    hip_check(hipStreamSynchronize(stream_), "sync");
    int a = 0, used = 0;
    for (int r = 0; r <= n_draft; ++r) {
        picks_out[r] = decide_row(vlogits_, r, opt, uniforms[used++]);
        a = r;
        if (r == n_draft || picks_out[r] != draft[r]) break;
    }
    if (draws_used) *draws_used = used;
    cache_len_ += a + 1;
    last_rows_ = rows;
    const int pos = cache_len_;
    hip_check(hipMemcpy(pos_, &pos, sizeof(int), hipMemcpyHostToDevice), "H2D pos");
    if (logits_out)
        hip_check(hipMemcpy(logits_out, vlogits_, (size_t)(n_draft + 1) * vocab * sizeof(float), hipMemcpyDeviceToHost), "D2H logits");
    return a;
}

std::vector<uint32_t> LlmModel::generate_lookup_sampled(const std::vector<uint32_t>& prompt, const GenerateOptions& opt, const LookupConfig& lk,
                                                        const std::function<bool(uint32_t)>& on_token, LookupStats* stats)
{
    if (stats) *stats = LookupStats();
    check_lookup_config(lk);
    if (opt.constraint) throw InvalidConfig("generate_lookup_sampled does not take a constraint (generate does)");
    if (opt.grammar) throw InvalidConfig("generate_lookup_sampled does not take a grammar (generate does)");
    if (opt.no_repeat_ngram > 0 || (!opt.sample && opt.repetition_penalty != 1.0f) || opt.logprobs >= 0)
        return generate(prompt, opt, on_token);  // not built (log-probabilities: the plain loop records them)
    if (!opt.sample) return generate_lookup(prompt, opt, lk, on_token, stats);
    DraftSource src;
    src.ngram_max = lk.ngram_max;
    src.ngram_min = lk.ngram_min;
    return sampled_draft_loop(prompt, opt, src, lk.draft_tokens, on_token, stats);
}

std::vector<uint32_t> LlmModel::sampled_draft_loop(const std::vector<uint32_t>& prompt, const GenerateOptions& opt, const DraftSource& src,
                                                   int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats)
{
    if (!opt.uniform) throw std::runtime_error("sampling needs a uniform source");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (prompt.empty()) throw std::runtime_error("cannot generate from empty prompt");
    if ((int)prompt.size() > cache_cap_) throw InvalidConfig("prompt does not fit the context");
    ensure_lookup_sampled();
    begin_sequence(prompt);
    drafter_begin(src, prompt);
    StreamScope on_this_stream(src.drafter, stream_);
    bool rounds_ran = false;
    const int vocab = cfg_.vocab;
    std::vector<uint32_t> out;
    GenerationRun run(prompt, opt, (size_t)cache_cap_, cfg_.eos_ids, out);
    const std::vector<uint32_t>& all = run.all;
    const bool penalty = opt.repetition_penalty != 1.0f;
    // generate()'s loop, one token: the checks ahead of the draw, the draw, the checks behind it.  False: the token did not join
    // the output (no draw was taken, or it was a stop token).  The picks of a step are the input rows of the next one, the last
    // token of the run is never one of them: the cache ends at all.size() - 1 rows, however the run ends.
    auto decide = [&](const float* logits_dev, int row, uint32_t* pick) {
        if (!run.wants_token()) return false;
        *pick = decide_row(logits_dev, row, opt, opt.uniform());
        return run.accept(*pick, on_token);
    };
    const size_t head_bytes = kLanes * sizeof(SampleHeader);
    if (!run.wants_token()) return out;
    // the device state: the history = the prompt (the picks join it step by step), the counts of the prompt, pos = history - 1
    LlmLookupState st = {};
    st.n = (int32_t)all.size();
    const int pos0 = cache_len_ - 1;
    hip_check(hipMemcpyAsync(lk_hist_, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_), "H2D history");
    hip_check(hipMemcpyAsync(lk_state_, &st, sizeof(st), hipMemcpyHostToDevice, stream_), "H2D lookup state");
    hip_check(hipMemcpyAsync(pos_, &pos0, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    if (penalty) begin_token_history(lk_hist_, nullptr, all.size(), samp_counts_, samp_distinct_, samp_ndistinct_);
    // the first token: the prompt's logits as a block of one row
    rows_cut(logits_, 1, opt);
    hip_check(hipMemcpyAsync(ls_host_, ls_out_, head_bytes + (size_t)kSampleRowsChunk * sizeof(SampleCandidate), hipMemcpyDeviceToHost, stream_),
              "D2H candidates");
    hip_check(hipStreamSynchronize(stream_), "sync");  // (`all` grows below: the copies must have read it)
    uint32_t picks[kLanes];
    int n_picks = decide(logits_, 0, &picks[0]) ? 1 : 0;
    while (run.wants_token()) {
        // as generate_lookup: a step of `rows` rows writes cache rows [pos, pos + rows); near the end of the cache the steps narrow
        const int room = cache_cap_ - cache_len_;
        if (room <= 0) break;
        const int rows = std::min(draft_tokens + 1, room);
        hipGraphExec_t exec = lookup_sampled_graph(rows, src, opt);
        ls_up_host_[0] = n_picks;
        for (int i = 0; i < n_picks; ++i) ls_up_host_[1 + i] = (int32_t)picks[i];
        hip_check(hipMemcpyAsync(ls_up_, ls_up_host_, 9 * sizeof(int32_t), hipMemcpyHostToDevice, stream_), "H2D picks");
        hip_check(launch_lookup_commit(ls_up_, lk_state_, lk_hist_, lk_hist_cap_, pos_, stream_), "lookup commit");
        if (penalty)
            hip_check(launch_token_counts(ls_up_ + 1, n_picks, vocab, samp_counts_, samp_distinct_, samp_ndistinct_, stream_), "token counts");
        hip_check(hipGraphLaunch(exec, stream_), "graph launch");
        rounds_ran = true;
        hip_check(hipMemcpyAsync(ls_host_, ls_out_, head_bytes + (size_t)rows * kSampleRowsChunk * sizeof(SampleCandidate),
                                 hipMemcpyDeviceToHost, stream_), "D2H candidates");
        if (src.drafter && rows > 1)  // a model's draft cannot be recomputed here: it comes back with the step's copy
            hip_check(hipMemcpyAsync(ls_draft_host_, vids_, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_), "D2H draft");
        hip_check(hipStreamSynchronize(stream_), "sync");
        // the draft the device made: a drafter's as copied, the lookup rule's from the same rule on the host's copy of the history
        std::vector<uint32_t> draft;
        if (src.drafter) {
            if (rows > 1) draft.assign(ls_draft_host_ + 1, ls_draft_host_ + rows);
        } else if (rows > 1) {
            LookupConfig hc;
            hc.ngram_max = src.ngram_max;
            hc.ngram_min = src.ngram_min;
            hc.draft_tokens = rows - 1;
            draft = lookup_draft_host(all.data(), all.size(), hc);
        }
        const int m = (int)draft.size();
        int a = 0;
        n_picks = 0;
        for (int r = 0; r <= m && run.wants_token(); ++r) {
            if (!decide(vlogits_, r, &picks[r])) break;
            ++n_picks;
            if (r == m || picks[r] != draft[(size_t)r]) break;
            ++a;
        }
        if (stats) stats->count(rows, m, a);
        cache_len_ = (int)all.size() - 1;
    }
    cache_len_ = (int)all.size() - 1;
    hip_check(hipMemcpy(pos_, &cache_len_, sizeof(int), hipMemcpyHostToDevice), "H2D pos");
    leave_resident(all);
    drafter_leave(src, all, rounds_ran);
    return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// Speculative decoding with a draft model (llm.h): the two loops above with a drafter as the draft source.

void LlmModel::check_draft_pair(const LlmModel* drafter, int draft_tokens) const
{
    if (!drafter) throw InvalidConfig("draft must not be null");
    if (drafter == this) throw InvalidConfig("draft must be another model than the decoder itself");
    if (drafter->device_ != device_)
        throw InvalidConfig("draft is on device " + std::to_string(drafter->device_) + ", the decoder on device " + std::to_string(device_));
    if (drafter->cfg_.vocab != cfg_.vocab)
        throw InvalidConfig("draft has a vocab of " + std::to_string(drafter->cfg_.vocab) + ", the decoder of " + std::to_string(cfg_.vocab));
    if (drafter->cache_cap_ < cache_cap_)
        throw InvalidConfig("draft has a context of " + std::to_string(drafter->cache_cap_) + " tokens, shorter than the decoder's " +
                            std::to_string(cache_cap_));
    if (draft_tokens < 1 || draft_tokens > kLookupMaxDraft) throw InvalidConfig("draft_tokens must be 1..7");
}

std::vector<uint32_t> LlmModel::generate_draft(LlmModel* drafter, const std::vector<uint32_t>& prompt, const GenerateOptions& opt,
                                               int draft_tokens, const std::function<bool(uint32_t)>& on_token, LookupStats* stats)
{
    if (stats) *stats = LookupStats();
    check_draft_pair(drafter, draft_tokens);
    if (opt.constraint) throw InvalidConfig("generate_draft does not take a constraint (generate does)");
    if (opt.grammar) throw InvalidConfig("generate_draft does not take a grammar (generate does)");
    if (prompt.empty()) throw InvalidConfig("prompt must not be empty");
    if (prompt.size() > (size_t)cache_cap_)
        throw InvalidConfig("prompt (" + std::to_string(prompt.size()) + " tokens) does not fit the context of " + std::to_string(cache_cap_) +
                            " tokens");
    if (opt.no_repeat_ngram > 0 || (!opt.sample && opt.repetition_penalty != 1.0f) || opt.logprobs >= 0)
        return generate(prompt, opt, on_token);  // not built (log-probabilities: the plain loop records them)
    DraftSource src;
    src.drafter = drafter;
    if (opt.sample) return sampled_draft_loop(prompt, opt, src, draft_tokens, on_token, stats);
    return greedy_draft_loop(prompt, opt, src, draft_tokens, on_token, stats);
}

int LlmModel::draft_round(LlmModel* drafter, uint32_t token, int rows, uint32_t* draft_out, uint32_t* tokens_out, float* logits_out)
{
    if (rows < 2 || rows > kLanes) throw InvalidConfig("rows must be 2..8");
    check_draft_pair(drafter, rows - 1);
    const int len = cache_len_;
    if (len < 1 || resident_.size() != (size_t)len)
        throw InvalidConfig("the decoder's resident tokens must cover its cache of at least one row");
    if (len + rows > cache_cap_)
        throw InvalidConfig("cache_len + rows (" + std::to_string(len) + " + " + std::to_string(rows) + ") exceeds the context of " +
                            std::to_string(cache_cap_) + " tokens");
    if (drafter->cache_len_ < len - 1 || drafter->resident_.size() < (size_t)(len - 1) ||
        !std::equal(resident_.begin(), resident_.begin() + (len - 1), drafter->resident_.begin()))
        throw InvalidConfig("draft does not hold the decoder's tokens up to cache_len - 1");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    ensure_lookup();
    drafter->ensure_lookup();
    StreamScope on_this_stream(drafter, stream_);
    const int32_t tail[2] = {(int32_t)resident_[(size_t)len - 1], (int32_t)token};
    LlmLookupState st = {};
    st.n = len + 1;
    hip_check(hipMemcpyAsync(lk_hist_ + (len - 1), tail, sizeof(tail), hipMemcpyHostToDevice, stream_), "H2D history");
    hip_check(hipMemcpyAsync(lk_state_, &st, sizeof(st), hipMemcpyHostToDevice, stream_), "H2D lookup state");
    hip_check(hipMemcpyAsync(pos_, &len, sizeof(int), hipMemcpyHostToDevice, stream_), "H2D pos");
    DraftSource src;
    src.drafter = drafter;
    enqueue_verify(rows, &src, false);
    uint32_t ids[kLanes];
    hip_check(hipMemcpyAsync(&st, lk_state_, sizeof(st), hipMemcpyDeviceToHost, stream_), "D2H lookup state");
    hip_check(hipMemcpyAsync(ids, vids_, sizeof(uint32_t) * (size_t)rows, hipMemcpyDeviceToHost, stream_), "D2H ids");
    hip_check(hipStreamSynchronize(stream_), "sync");
    const int a = st.a, m = rows - 1;
    for (int i = 0; i < m; ++i) draft_out[i] = ids[1 + i];
    for (int i = 0; i <= a; ++i) tokens_out[i] = (uint32_t)st.picks[i];
    resident_.push_back(token);
    for (int i = 0; i < a; ++i) resident_.push_back(tokens_out[i]);
    cache_len_ = len + a + 1;
    last_rows_ = rows;
    // the drafter computed rows for T[len - 1], the token and drafts 1 .. m - 1: valid through draft min(a, m - 1)
    drafter->cache_len_ = len + 1 + std::min(a, m - 1);
    drafter->last_rows_ = 1;
    drafter->resident_.assign(resident_.begin(), resident_.begin() + drafter->cache_len_);
    hip_check(hipMemcpy(drafter->pos_, &drafter->cache_len_, sizeof(int), hipMemcpyHostToDevice), "H2D pos");
    if (logits_out)
        hip_check(hipMemcpy(logits_out, vlogits_, (size_t)rows * cfg_.vocab * sizeof(float), hipMemcpyDeviceToHost), "D2H logits");
    return a;
}

// ---- embedding ----------------------------------------------------------------------------------------------------------------

std::vector<EmbedChunk> embed_plan_host(const int32_t* lengths, int n, int head_dim)
{
    std::vector<EmbedChunk> chunks;
    for (int i = 0; i < n; ++i) {
        const int len = lengths[i];
        if (len < 1 || len > kEmbedChunkRows)
            throw InvalidConfig("lengths[" + std::to_string(i) + "] = " + std::to_string(len) + " is outside 1 .. " +
                                std::to_string(kEmbedChunkRows));
        if (chunks.empty() || chunks.back().rows + len > kEmbedChunkRows) {
            chunks.emplace_back();
            chunks.back().first_seq = i;
        }
        EmbedChunk& c = chunks.back();
        const bool mfma = embed_seq_takes_mfma(len, head_dim);
        const int step = mfma ? 128 : 32;
        for (int q0 = 0; q0 < len; q0 += step) (mfma ? c.mfma : c.vec).push_back(EmbedBlock{c.rows, q0, len});
        c.rows += len;
        ++c.n_seq;
    }
    return chunks;
}

namespace {

// A chunk's metadata on the device.  embed_batch: ids [m] | row_pos [m] | seq_start [n + 1] | vec blocks | mfma blocks with
// m <= 2048 rows, n <= 2048 sequences, at most m / 32 + n vec blocks and m / 128 + n / 256 + 1 mfma blocks of 3 words.
// score_batch: ids [m] | row_pos [m] | gather rows [g] | targets [g] | vec | mfma | prefix blocks with g < m scored positions, at
// most m blocks in the vec and in the prefix table (a block has at least one row of its own) of 3 and 5 words.
constexpr size_t kPackedMetaWords = 4 * (size_t)kEmbedChunkRows + 3 * (size_t)kEmbedChunkRows + 3 * 32 + 5 * (size_t)kEmbedChunkRows + 8;

// The sequences of a packed call, b = ids[offsets[b], offsets[b + 1]): InvalidConfig naming the argument and the sequence for
// B < 0, decreasing offsets, a sequence shorter than min_len (1 or 2) or longer than `limit`, and an id >= vocab (ids null: not
// checked).  `noun` is the entry's word in the messages: embed, score or answer.
void check_packed_sequences(const char* noun, const uint32_t* ids, const int32_t* offsets, int B, int min_len, int limit, int vocab)
{
    if (B < 0) throw InvalidConfig("n_sequences (" + std::to_string(B) + ") is negative");
    if (B == 0) return;
    if (offsets[0] < 0) throw InvalidConfig("offsets[0] = " + std::to_string(offsets[0]) + " is negative (sequence 0)");
    for (int b = 0; b < B; ++b) {
        const int64_t len = (int64_t)offsets[b + 1] - offsets[b];
        const std::string seq = " (sequence " + std::to_string(b) + ")";
        if (len < 0) throw InvalidConfig("offsets[" + std::to_string(b + 1) + "] = " + std::to_string(offsets[b + 1]) + " is below offsets[" +
                                         std::to_string(b) + "] = " + std::to_string(offsets[b]) + ": offsets must not decrease" + seq);
        if (len == 0 && min_len == 1)
            throw InvalidConfig("offsets[" + std::to_string(b) + "] == offsets[" + std::to_string(b + 1) + "]: an empty sequence" + seq);
        if (len < min_len)  // (score's own words say why)
            throw InvalidConfig("offsets: " + std::to_string(len) + " tokens are fewer than " + std::to_string(min_len) +
                                (std::strcmp(noun, "score") == 0 ? ": a scored token needs a prefix" : "") + seq);
        if (len > limit)
            throw InvalidConfig("offsets: " + std::to_string(len) + " tokens exceed the " + noun + " length limit of " + std::to_string(limit) + seq);
        for (int32_t i = offsets[b]; ids && i < offsets[b + 1]; ++i)
            if (ids[i] >= (uint32_t)vocab)
                throw InvalidConfig("ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is not below the vocabulary size " +
                                    std::to_string(vocab) + seq);
    }
}

}  // namespace

void LlmModel::ensure_packed_scratch()
{
    if (ek_) return;
    const int kv = cfg_.kv_heads * cfg_.head_dim;
    ek_ = dalloc((size_t)kEmbedChunkRows * kv);
    ev_ = dalloc((size_t)kEmbedChunkRows * kv);
    emeta_ = reinterpret_cast<int32_t*>(dalloc(kPackedMetaWords));
    hip_check(hipHostMalloc((void**)&emeta_host_, kPackedMetaWords * sizeof(int32_t), hipHostMallocDefault), "hipHostMalloc");
}

LlmModel::PackedMeta LlmModel::upload_packed_meta(const char* entry, int m, const uint32_t* ids, const int32_t* row_tok, const int32_t* row_pos,
                                                  const void* extra_a, size_t n_a, const void* extra_b, size_t n_b,
                                                  const std::vector<EmbedBlock>& vec, const std::vector<EmbedBlock>& mfma,
                                                  const std::vector<PrefixBlock>& prefix)
{
    const size_t o_pos = (size_t)m, o_a = o_pos + (size_t)m, o_b = o_a + n_a, o_vec = o_b + n_b, o_mfma = o_vec + 3 * vec.size();
    const size_t o_pre = o_mfma + 3 * mfma.size(), words = o_pre + 5 * prefix.size();
    static_assert(sizeof(EmbedBlock) == 3 * sizeof(int32_t) && sizeof(PrefixBlock) == 5 * sizeof(int32_t), "the block tables' words");
    if (words > kPackedMetaWords) throw std::runtime_error(std::string(entry) + ": chunk metadata exceeds its buffer");
    int32_t* hm = emeta_host_;
    if (row_tok)
        for (int r = 0; r < m; ++r) hm[r] = (int32_t)ids[row_tok[r]];
    else std::memcpy(hm, ids, (size_t)m * 4);
    std::memcpy(hm + o_pos, row_pos, (size_t)m * 4);
    if (n_a) std::memcpy(hm + o_a, extra_a, n_a * 4);
    if (n_b) std::memcpy(hm + o_b, extra_b, n_b * 4);
    if (!vec.empty()) std::memcpy(hm + o_vec, vec.data(), vec.size() * sizeof(EmbedBlock));
    if (!mfma.empty()) std::memcpy(hm + o_mfma, mfma.data(), mfma.size() * sizeof(EmbedBlock));
    if (!prefix.empty()) std::memcpy(hm + o_pre, prefix.data(), prefix.size() * sizeof(PrefixBlock));
    hip_check(hipMemcpyAsync(emeta_, hm, words * 4, hipMemcpyHostToDevice, stream_), "H2D chunk");
    return PackedMeta{reinterpret_cast<const uint32_t*>(emeta_), emeta_ + o_pos, emeta_ + o_a, emeta_ + o_b,
                      reinterpret_cast<const EmbedBlock*>(emeta_ + o_vec), reinterpret_cast<const EmbedBlock*>(emeta_ + o_mfma),
                      reinterpret_cast<const PrefixBlock*>(emeta_ + o_pre)};
}

void LlmModel::packed_layers(int m, const uint32_t* ids_dev, const int32_t* row_pos, const EmbedBlock* vec, int nv, const EmbedBlock* mfma,
                             int nm, const PrefixBlock* prefix, int np)
{
    const LlmConfig& c = cfg_;
    const int d = c.head_dim, kv = c.kv_heads * d, QD = c.q_dim();
    hipStream_t s = stream_;
    embed_rows(ids_dev, m, ph_, 0, nullptr, row_pos);
    for (const Layer& L : layers_) {
        rows_qkv(m, L, ek_, ev_);
        if (c.qwen3()) {
            hip_check(launch_qk_norm_rope_rows(pq_, QD, ek_, kv, m, c.heads, c.kv_heads, d, L.q_norm, L.k_norm, c.eps, cos_, sin_, row_pos, s),
                      "qk norm + rope");
        } else if (!gpt2_) {  // (GPT-2: learned positions, already in the embedding)
            hip_check(launch_rope_rows(pq_, QD, m, c.heads, d, cos_, sin_, row_pos, s), "rope q");
            hip_check(launch_rope_rows(ek_, kv, m, c.kv_heads, d, cos_, sin_, row_pos, s), "rope k");
        }
        hip_check(launch_packed_causal_attention(pq_, QD, ek_, kv, ev_, kv, vec, nv, mfma, nm, c.heads, d, c.heads / c.kv_heads, pctx_, QD, s),
                  "packed attention");
        hip_check(launch_packed_prefix_attention(pq_, QD, ek_, kv, ev_, kv, prefix, np, c.heads, d, c.heads / c.kv_heads, pctx_, QD, s),
                  "packed prefix attention");
        rows_finish(m, L);
    }
}

void LlmModel::embed_batch(const uint32_t* ids, const int32_t* offsets, int B, bool normalize, float* out)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden;
    if (gpt2_) throw InvalidConfig("embed: GPT-2 has no RMSNorm layer stack and is no embedding family");
    if (quant_) throw InvalidConfig("embed: quantized checkpoints are not supported");
    if (!packed_geometry(c)) throw InvalidConfig(packed_geometry_refusal("embed"));
    check_packed_sequences("embed", ids, offsets, B, 1, embed_max_tokens(), c.vocab);
    if (B == 0) return;
    std::vector<int32_t> lengths((size_t)B);
    for (int b = 0; b < B; ++b) lengths[(size_t)b] = offsets[b + 1] - offsets[b];
    const std::vector<EmbedChunk> chunks = embed_plan_host(lengths.data(), B, c.head_dim);

    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipStream_t s = stream_;
    ensure_prompt_workspace();
    ensure_packed_scratch();
    std::vector<int32_t> row_pos, seq_start;
    for (const EmbedChunk& ch : chunks) {
        const int m = ch.rows, n = ch.n_seq;
        row_pos.clear();
        seq_start.clear();
        for (int j = 0; j < n; ++j) {
            seq_start.push_back((int32_t)row_pos.size());
            for (int t = 0; t < lengths[(size_t)(ch.first_seq + j)]; ++t) row_pos.push_back(t);
        }
        seq_start.push_back((int32_t)row_pos.size());
        const PackedMeta meta = upload_packed_meta("embed", m, ids + offsets[ch.first_seq], nullptr, row_pos.data(), seq_start.data(),
                                                   seq_start.size(), nullptr, 0, ch.vec, ch.mfma, {});
        packed_layers(m, meta.ids, meta.row_pos, meta.vec, (int)ch.vec.size(), meta.mfma, (int)ch.mfma.size(), nullptr, 0);
        // (the norm buffer is free after the last layer: the pooled rows land there)
        hip_check(launch_last_token_pool(ph_, H, meta.extra_a, n, H, final_norm_, c.eps, normalize ? 1 : 0, pn_, s), "last-token pool");
        hip_check(hipMemcpyAsync(out + (size_t)ch.first_seq * H, pn_, (size_t)n * H * sizeof(float), hipMemcpyDeviceToHost, s), "D2H embeddings");
        hip_check(hipStreamSynchronize(s), "sync");  // the staging copy and the activations are reused by the next chunk
    }
}

// ---- scoring many sequences in one packed pass -------------------------------------------------------------------------------

namespace {

// firsts of score_plan_host and score_batch, behind check_packed_sequences: InvalidConfig naming the argument and the sequence
void check_firsts(const int32_t* offsets, const int32_t* firsts, int B)
{
    for (int b = 0; b < B; ++b) {
        const int32_t len = offsets[b + 1] - offsets[b];
        if (firsts[b] < 1 || firsts[b] >= len)
            throw InvalidConfig("firsts[" + std::to_string(b) + "] = " + std::to_string(firsts[b]) + " must be in [1, " + std::to_string(len) +
                                ") (sequence " + std::to_string(b) + ")");
    }
}

}  // namespace

ScorePlan score_plan_host(const uint32_t* ids, const int32_t* offsets, const int32_t* firsts, int B, int head_dim, int min_shared)
{
    check_packed_sequences("score", nullptr, offsets, B, 2, kEmbedChunkRows, 0);
    check_firsts(offsets, firsts, B);
    if (min_shared < 1) throw InvalidConfig("min_shared (" + std::to_string(min_shared) + ") must be at least 1");
    ScorePlan plan;
    auto len_of = [&](int b) { return offsets[b + 1] - offsets[b]; };
    auto lcp = [&](int a, int b, int cap) {  // common prefix of sequences a and b, at most cap
        const uint32_t *x = ids + offsets[a], *y = ids + offsets[b];
        const int n = std::min(cap, std::min(len_of(a), len_of(b)));
        int k = 0;
        while (k < n && x[k] == y[k]) ++k;
        return k;
    };
    std::vector<int64_t> slot0((size_t)B + 1, 0);  // a sequence's first slot in the flat outputs
    for (int b = 0; b < B; ++b) slot0[(size_t)b + 1] = slot0[(size_t)b] + (len_of(b) - firsts[b]);
    auto add_blocks = [&](ScoreChunk& c, int first_row, int len) {  // embed_plan_host's rule
        const bool mf = embed_seq_takes_mfma(len, head_dim);
        for (int q0 = 0; q0 < len; q0 += mf ? 128 : 32) (mf ? c.mfma : c.vec).push_back(EmbedBlock{first_row, q0, len});
    };
    int i = 0;
    while (i < B) {
        int p = firsts[i], j = i + 1;
        int64_t rest = len_of(i);  // sum of the members' lengths
        int longest = len_of(i);
        while (j < B) {
            const int q = lcp(i, j, std::min(p, firsts[j]));  // a shared prefix never contains a scored token
            if (q < min_shared) break;
            const int64_t total = rest + len_of(j);
            const int n_mem = j - i + 1;
            if (q + (total - (int64_t)n_mem * q) > kEmbedChunkRows) break;  // a group lives in one chunk
            if (std::max(longest, len_of(j)) - q >= 256) break;             // remainders take the 32-query route only
            p = q;
            rest = total;
            longest = std::max(longest, len_of(j));
            ++j;
        }
        const bool group = j - i >= 2;
        if (!group) {
            p = 0;
            j = i + 1;
        }
        const int n_mem = j - i;
        int cost = p;
        for (int t = i; t < j; ++t) cost += len_of(t) - p;
        if (plan.chunks.empty() || plan.chunks.back().rows + cost > kEmbedChunkRows) {
            plan.chunks.emplace_back();
            plan.chunks.back().first_seq = i;
        }
        ScoreChunk& c = plan.chunks.back();
        const int prefix_first = c.rows;
        if (group) {
            plan.groups.push_back(ScoreGroup{(int)plan.chunks.size() - 1, i, n_mem, p});
            plan.saved += (int64_t)(n_mem - 1) * p;
            add_blocks(c, prefix_first, p);
            for (int r = 0; r < p; ++r) {
                c.row_tok.push_back(offsets[i] + r);
                c.row_pos.push_back(r);
            }
            c.rows += p;
        }
        for (int t = i; t < j; ++t) {
            const int len = len_of(t), own = len - p, first_row = c.rows;
            if (group) {
                for (int q0 = 0; q0 < own; q0 += 32) c.prefix.push_back(PrefixBlock{first_row, q0, own, prefix_first, p});
            } else {
                add_blocks(c, first_row, own);
            }
            for (int r = p; r < len; ++r) {
                c.row_tok.push_back(offsets[t] + r);
                c.row_pos.push_back(r);
            }
            for (int pos = firsts[t]; pos < len; ++pos) {  // position pos - 1: the prefix's last row when it is p - 1
                c.gather_src.push_back(pos - 1 >= p ? first_row + (pos - 1 - p) : prefix_first + p - 1);
                c.gather_tgt.push_back((int32_t)ids[offsets[t] + pos]);
                c.gather_slot.push_back((int32_t)(slot0[(size_t)t] + (pos - firsts[t])));
            }
            c.rows += own;
        }
        c.n_seq += n_mem;
        plan.rows += cost;
        i = j;
    }
    return plan;
}

bool LlmModel::score_batch_supported() const { return !quant_ && packed_geometry(cfg_); }

void LlmModel::score_batch(const uint32_t* ids, const int32_t* offsets, int B, const int32_t* firsts, int top_k, float* logprob_out,
                           uint32_t* topk_ids_out, float* topk_logprob_out)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden;
    if (quant_) throw InvalidConfig("score_batch: quantized checkpoints are not supported");
    if (!packed_geometry(c)) throw InvalidConfig(packed_geometry_refusal("score_batch"));
    if (top_k < 1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > c.vocab)
        throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [1, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                            "] and not above the vocabulary size " + std::to_string(c.vocab));
    check_packed_sequences("score", ids, offsets, B, 2, embed_max_tokens(), c.vocab);
    check_firsts(offsets, firsts, B);
    if (B == 0) return;
    const ScorePlan plan = score_plan_host(ids, offsets, firsts, B, c.head_dim, kScoreMinShared);

    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipStream_t s = stream_;
    ensure_prompt_workspace();
    ensure_packed_scratch();
    ensure_score();  // the slab scratch of the fused head
    if (top_k > 1) ensure_score_topk();
    constexpr size_t kResWords = (size_t)kEmbedChunkRows * (1 + 2 * KJARNI_SCORE_TOPK_MAX);
    if (!sb_res_) {
        sb_res_ = reinterpret_cast<uint32_t*>(dalloc(kResWords));
        hip_check(hipHostMalloc((void**)&sb_res_host_, kResWords * sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc");
    }
    for (const ScoreChunk& ch : plan.chunks) {
        const int m = ch.rows, g = (int)ch.gather_src.size();
        if (g > kEmbedChunkRows) throw std::runtime_error("score_batch: chunk metadata exceeds its buffer");  // (sb_res_ holds 2 048 rows)
        const PackedMeta meta = upload_packed_meta("score_batch", m, ids, ch.row_tok.data(), ch.row_pos.data(), ch.gather_src.data(), (size_t)g,
                                                   ch.gather_tgt.data(), (size_t)g, ch.vec, ch.mfma, ch.prefix);
        packed_layers(m, meta.ids, meta.row_pos, meta.vec, (int)ch.vec.size(), meta.mfma, (int)ch.mfma.size(), meta.prefix, (int)ch.prefix.size());
        // (the norm buffer is free after the last layer: the gathered rows land there, compact, H floats apart)
        hip_check(launch_score_gather_norm(ph_, H, meta.extra_a, g, H, final_norm_, gpt2_ ? final_norm_b_ : nullptr, c.eps, pn_, H, s),
                  "score gather + norm");
        // the chunk's results: logprob [g] | top-k ids [g, top_k] | top-k logprob [g, top_k]; top_k 1 is score()'s plain head
        score_head(pn_, g, reinterpret_cast<const uint32_t*>(meta.extra_b), top_k > 1 ? top_k : 0, reinterpret_cast<float*>(sb_res_), sb_res_ + g,
                   reinterpret_cast<float*>(sb_res_ + g + (size_t)g * top_k));
        const size_t res_words = (size_t)g * (1 + 2 * (size_t)top_k);
        hip_check(hipMemcpyAsync(sb_res_host_, sb_res_, res_words * 4, hipMemcpyDeviceToHost, s), "D2H scores");
        hip_check(hipStreamSynchronize(s), "sync");  // the staging copies and the activations are reused by the next chunk
        const size_t slot = (size_t)ch.gather_slot[0];  // (a chunk's slots are consecutive: sequence order, then position order)
        if (logprob_out) std::memcpy(logprob_out + slot, sb_res_host_, (size_t)g * 4);
        if (topk_ids_out) std::memcpy(topk_ids_out + slot * top_k, sb_res_host_ + g, (size_t)g * top_k * 4);
        if (topk_logprob_out) std::memcpy(topk_logprob_out + slot * top_k, sb_res_host_ + g + (size_t)g * top_k, (size_t)g * top_k * 4);
    }
    score_batch_rows_ += (uint64_t)plan.rows;
    score_batch_saved_ += (uint64_t)plan.saved;
}

// ---- answer logits: a few chosen logits at the end of many sequences ----------------------------------------------------------

ScorePlan answer_plan_host(const uint32_t* ids, const int32_t* offsets, int B, int head_dim, int min_shared)
{
    // the one scored position of a sequence is its last token: score_plan_host's rule then keeps that token out of every prefix
    std::vector<int32_t> firsts((size_t)std::max(B, 0));
    for (int b = 0; b < B; ++b) firsts[(size_t)b] = (int32_t)std::max<int64_t>((int64_t)offsets[b + 1] - offsets[b] - 1, 1);
    ScorePlan plan = score_plan_host(ids, offsets, firsts.data(), B, head_dim, min_shared);
    for (ScoreChunk& c : plan.chunks) {
        // rows and sequences both run in order, and a last token is a row of its sequence alone
        c.gather_src.clear();
        c.gather_tgt.clear();
        c.gather_slot.clear();
        int t = c.first_seq;
        for (int r = 0; r < c.rows && t < c.first_seq + c.n_seq; ++r)
            if (c.row_tok[(size_t)r] == offsets[t + 1] - 1) {
                c.gather_src.push_back(r);
                c.gather_slot.push_back(t++);
            }
        if ((int)c.gather_src.size() != c.n_seq) throw std::runtime_error("answer plan: a sequence's last token has no row");
    }
    return plan;
}

void LlmModel::answer_logits_batch(const uint32_t* ids, const int32_t* offsets, int B, const uint32_t* targets, int n_targets,
                                   float* logits_out)
{
    const LlmConfig& c = cfg_;
    const int H = c.hidden;
    if (quant_) throw InvalidConfig("answer_logits: quantized checkpoints are not supported");
    if (!packed_geometry(c)) throw InvalidConfig(packed_geometry_refusal("answer_logits"));
    if (n_targets < 1 || n_targets > kAnswerMaxTargets)
        throw InvalidConfig("n_targets (" + std::to_string(n_targets) + ") must be in [1, " + std::to_string(kAnswerMaxTargets) + "]");
    for (int t = 0; t < n_targets; ++t)
        if (targets[t] >= (uint32_t)c.vocab)
            throw InvalidConfig("targets[" + std::to_string(t) + "] = " + std::to_string(targets[t]) + " is not below the vocabulary size " +
                                std::to_string(c.vocab));
    check_packed_sequences("answer", ids, offsets, B, 2, embed_max_tokens(), c.vocab);
    if (B == 0) return;
    const ScorePlan plan = answer_plan_host(ids, offsets, B, c.head_dim, kScoreMinShared);

    hip_check(hipSetDevice(device_), "hipSetDevice");
    hipStream_t s = stream_;
    ensure_prompt_workspace();
    ensure_packed_scratch();
    for (const ScoreChunk& ch : plan.chunks) {
        const int m = ch.rows, n = ch.n_seq;
        const PackedMeta meta = upload_packed_meta("answer_logits", m, ids, ch.row_tok.data(), ch.row_pos.data(), ch.gather_src.data(), (size_t)n,
                                                   targets, (size_t)n_targets, ch.vec, ch.mfma, ch.prefix);
        packed_layers(m, meta.ids, meta.row_pos, meta.vec, (int)ch.vec.size(), meta.mfma, (int)ch.mfma.size(), meta.prefix, (int)ch.prefix.size());
        // (the norm buffer is free after the last layer: the chunk's [n, n_targets] logits land there)
        hip_check(launch_answer_logits(ph_, H, meta.extra_a, n, H, final_norm_, gpt2_ ? final_norm_b_ : nullptr, c.eps, lm_head_, bf16_ ? 1 : 0,
                                       reinterpret_cast<const uint32_t*>(meta.extra_b), n_targets, pn_, s), "answer logits");
        // They land in the pinned staging buffer, as score_batch's results land in a pinned one: the chunk's upload from it is
        // behind us on the stream, and n * n_targets <= 1 024 * 8 words fit it.
        static_assert((size_t)(kEmbedChunkRows / 2) * kAnswerMaxTargets <= kPackedMetaWords, "a chunk's logits fit the staging buffer");
        hip_check(hipMemcpyAsync(emeta_host_, pn_, (size_t)n * n_targets * sizeof(float), hipMemcpyDeviceToHost, s), "D2H answer logits");
        hip_check(hipStreamSynchronize(s), "sync");  // the staging copy and the activations are reused by the next chunk
        // (a chunk's sequences are consecutive: its logits are one block of the output)
        std::memcpy(logits_out + (size_t)ch.first_seq * n_targets, emeta_host_, (size_t)n * n_targets * sizeof(float));
    }
    answer_rows_ += (uint64_t)plan.rows;
    answer_saved_ += (uint64_t)plan.saved;
}

}  // namespace kjarni
