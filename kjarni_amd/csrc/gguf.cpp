#include "gguf.h"

#include <dirent.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>

// Dequantization must round exactly as the reference's scalar code does: no fused multiply-adds on the host side.
#pragma clang fp contract(off)

namespace kjarni {

namespace {

float half_to_f32(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    uint32_t u;
    if (exp == 0) {
        if (man == 0) {
            u = sign;
        } else {  // subnormal half: normalise
            int e = -1;
            uint32_t m = man;
            do {
                ++e;
                m <<= 1;
            } while (!(m & 0x400u));
            u = sign | ((uint32_t)(127 - 15 - e) << 23) | ((m & 0x3FFu) << 13);
        }
    } else if (exp == 31) {
        u = sign | 0x7F800000u | (man << 13);
    } else {
        u = sign | ((exp + 127 - 15) << 23) | (man << 13);
    }
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

void scale_min_k4(int j, const uint8_t* q, uint8_t* sc, uint8_t* m)  // get_scale_min_k4 (q_common.rs)
{
    if (j < 4) {
        *sc = q[j] & 63;
        *m = q[j + 4] & 63;
    } else {
        *sc = (uint8_t)((q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4));
        *m = (uint8_t)((q[j + 4] >> 4) | ((q[j] >> 6) << 4));
    }
}

struct Reader {
    const uint8_t* p;
    size_t size, pos = 0;
    void need(size_t n, const char* what) const
    {
        if (n > size - pos) throw std::runtime_error(std::string("GGUF: file is truncated (") + what + ")");
    }
    template <class T>
    T get(const char* what)
    {
        need(sizeof(T), what);
        T v;
        std::memcpy(&v, p + pos, sizeof(T));
        pos += sizeof(T);
        return v;
    }
    std::string str(const char* what)
    {
        const uint64_t n = get<uint64_t>(what);
        if (n > size - pos) throw std::runtime_error(std::string("GGUF: file is truncated (") + what + ")");
        std::string s(reinterpret_cast<const char*>(p + pos), (size_t)n);
        pos += (size_t)n;
        return s;
    }
};

size_t scalar_size(uint32_t t)
{
    switch (t) {
    case 0: case 1: case 7: return 1;
    case 2: case 3: return 2;
    case 4: case 5: case 6: return 4;
    case 10: case 11: case 12: return 8;
    default: return 0;
    }
}

void skip_value(Reader& r, uint32_t t, int depth)
{
    if (t == 8) {
        (void)r.str("metadata string");
    } else if (t == 9) {
        if (depth > 4) throw std::runtime_error("GGUF: metadata arrays nested too deeply");
        const uint32_t et = r.get<uint32_t>("array type");
        const uint64_t n = r.get<uint64_t>("array length");
        const size_t es = scalar_size(et);
        if (es) {
            if (n > (r.size - r.pos) / es) throw std::runtime_error("GGUF: file is truncated (metadata array)");
            r.pos += (size_t)n * es;
        } else if (et == 8 || et == 9) {
            if (n > (r.size - r.pos) / 8) throw std::runtime_error("GGUF: file is truncated (metadata array)");
            for (uint64_t i = 0; i < n; ++i) skip_value(r, et, depth + 1);
        } else {
            throw std::runtime_error("GGUF: unknown metadata array element type " + std::to_string(et));
        }
    } else {
        const size_t es = scalar_size(t);
        if (!es) throw std::runtime_error("GGUF: unknown metadata value type " + std::to_string(t));
        r.need(es, "metadata value");
        r.pos += es;
    }
}

// HF name -> GGUF name (gguf_loader.rs:151-187; Qwen2's q/k/v biases as llama.cpp names them)
std::string to_gguf_name(const std::string& name)
{
    if (name == "model.embed_tokens.weight") return "token_embd.weight";
    if (name == "model.norm.weight") return "output_norm.weight";
    if (name == "lm_head.weight") return "output.weight";
    static const char* kPrefix = "model.layers.";
    if (name.compare(0, 13, kPrefix) == 0) {
        const size_t dot = name.find('.', 13);
        if (dot == std::string::npos) return name;
        const std::string layer = name.substr(13, dot - 13), suffix = name.substr(dot + 1);
        static const std::pair<const char*, const char*> kMap[] = {
            {"input_layernorm.weight", "attn_norm.weight"},       {"self_attn.q_proj.weight", "attn_q.weight"},
            {"self_attn.k_proj.weight", "attn_k.weight"},         {"self_attn.v_proj.weight", "attn_v.weight"},
            {"self_attn.o_proj.weight", "attn_output.weight"},    {"post_attention_layernorm.weight", "ffn_norm.weight"},
            {"mlp.gate_proj.weight", "ffn_gate.weight"},          {"mlp.up_proj.weight", "ffn_up.weight"},
            {"mlp.down_proj.weight", "ffn_down.weight"},          {"self_attn.q_proj.bias", "attn_q.bias"},
            {"self_attn.k_proj.bias", "attn_k.bias"},             {"self_attn.v_proj.bias", "attn_v.bias"},
        };
        for (const auto& m : kMap)
            if (suffix == m.first) return "blk." + layer + "." + m.second;
        return "blk." + layer + "." + suffix;
    }
    return name;
}

bool ends_with(const std::string& s, const std::string& tail)
{
    return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0;
}

bool is_file(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

bool is_dir(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

std::string fmt_float(double v)
{
    char b[64];
    std::snprintf(b, sizeof b, "%.9g", v);
    std::string s(b);
    if (s.find_first_of(".eEn") == std::string::npos) s += ".0";
    return s;
}

}  // namespace

float f16_to_f32(uint16_t h) { return half_to_f32(h); }

void q4k_scale_min(int j, const uint8_t* scales, uint8_t* sc, uint8_t* m) { scale_min_k4(j, scales, sc, m); }

const char* ggml_type_name(uint32_t type)
{
    switch (type) {
    case GGML_F32: return "F32";
    case GGML_F16: return "F16";
    case GGML_Q4_0: return "Q4_0";
    case GGML_Q4_1: return "Q4_1";
    case GGML_Q5_0: return "Q5_0";
    case GGML_Q5_1: return "Q5_1";
    case GGML_Q8_0: return "Q8_0";
    case 9: return "Q8_1";
    case 10: return "Q2_K";
    case 11: return "Q3_K";
    case GGML_Q4_K: return "Q4_K";
    case GGML_Q5_K: return "Q5_K";
    case GGML_Q6_K: return "Q6_K";
    case 15: return "Q8_K";
    case GGML_BF16: return "BF16";
    default: return "unknown";
    }
}

bool ggml_block_geometry(uint32_t type, int64_t* elems, int64_t* bytes)
{
    switch (type) {
    case GGML_F32: *elems = 1; *bytes = 4; return true;
    case GGML_Q4_0: *elems = 32; *bytes = 18; return true;
    case GGML_Q4_1: *elems = 32; *bytes = 20; return true;
    case GGML_Q5_0: *elems = 32; *bytes = 22; return true;
    case GGML_Q5_1: *elems = 32; *bytes = 24; return true;
    case GGML_Q8_0: *elems = 32; *bytes = 34; return true;
    case GGML_Q4_K: *elems = 256; *bytes = 144; return true;
    case GGML_Q5_K: *elems = 256; *bytes = 176; return true;
    case GGML_Q6_K: *elems = 256; *bytes = 210; return true;
    default: return false;
    }
}

void ggml_dequantize_row(uint32_t type, const uint8_t* src, int64_t n, float* out)
{
    switch (type) {
    case GGML_F32:
        std::memcpy(out, src, (size_t)n * 4);
        return;
    case GGML_Q8_0:
        for (int64_t b = 0; b < n / 32; ++b, src += 34, out += 32) {
            const float d = half_to_f32(rd16(src));
            for (int i = 0; i < 32; ++i) out[i] = (float)(int8_t)src[2 + i] * d;
        }
        return;
    case GGML_Q4_K:
        for (int64_t b = 0; b < n / 256; ++b, src += 144, out += 256) {
            const float d = half_to_f32(rd16(src)), dmin = half_to_f32(rd16(src + 2));
            const uint8_t *sc = src + 4, *qs = src + 16;
            for (int j = 0; j < 4; ++j) {
                uint8_t s1, m1, s2, m2;
                scale_min_k4(2 * j, sc, &s1, &m1);
                scale_min_k4(2 * j + 1, sc, &s2, &m2);
                const float d1 = d * (float)s1, mn1 = dmin * (float)m1, d2 = d * (float)s2, mn2 = dmin * (float)m2;
                for (int l = 0; l < 32; ++l) out[j * 64 + l] = d1 * (float)(qs[j * 32 + l] & 0xF) - mn1;
                for (int l = 0; l < 32; ++l) out[j * 64 + 32 + l] = d2 * (float)(qs[j * 32 + l] >> 4) - mn2;
            }
        }
        return;
    case GGML_Q4_0:
    case GGML_Q4_1:
    case GGML_Q5_0:
    case GGML_Q5_1: {
        // d (, m) (, qh u32), qs[16]: element e < 16 is the low nibble of qs[e], element 16 + e the high one; bit e of qh is
        // element e's fifth bit.  Every product is exact in f32, so each weight is rounded once (in the add) or not at all.
        const bool has_m = type == GGML_Q4_1 || type == GGML_Q5_1, has_h = type == GGML_Q5_0 || type == GGML_Q5_1;
        const int qh_at = has_m ? 4 : 2, qs_at = qh_at + (has_h ? 4 : 0), bytes = qs_at + 16;
        const int off = has_m ? 0 : (has_h ? 16 : 8);
        for (int64_t b = 0; b < n / 32; ++b, src += bytes, out += 32) {
            const float d = half_to_f32(rd16(src)), m = has_m ? half_to_f32(rd16(src + 2)) : 0.0f;
            uint32_t qh = 0;
            if (has_h) std::memcpy(&qh, src + qh_at, 4);
            const uint8_t* qs = src + qs_at;
            for (int e = 0; e < 32; ++e) {
                const int nib = e < 16 ? (qs[e] & 0xF) : (qs[e - 16] >> 4);
                const int q = nib | (int)(((qh >> e) & 1u) << 4);
                out[e] = has_m ? (float)q * d + m : (float)(q - off) * d;
            }
        }
        return;
    }
    case GGML_Q5_K:
        for (int64_t b = 0; b < n / 256; ++b, src += 176, out += 256) {
            const float d = half_to_f32(rd16(src)), dmin = half_to_f32(rd16(src + 2));
            const uint8_t *sc = src + 4, *qh = src + 16, *qs = src + 48;
            for (int j = 0; j < 4; ++j) {
                uint8_t s1, m1, s2, m2;
                scale_min_k4(2 * j, sc, &s1, &m1);
                scale_min_k4(2 * j + 1, sc, &s2, &m2);
                const float d1 = d * (float)s1, mn1 = dmin * (float)m1, d2 = d * (float)s2, mn2 = dmin * (float)m2;
                for (int l = 0; l < 32; ++l) {
                    const int lo = (qs[j * 32 + l] & 0xF) | (((qh[l] >> (2 * j)) & 1) << 4);
                    const int hi = (qs[j * 32 + l] >> 4) | (((qh[l] >> (2 * j + 1)) & 1) << 4);
                    out[j * 64 + l] = d1 * (float)lo - mn1;
                    out[j * 64 + 32 + l] = d2 * (float)hi - mn2;
                }
            }
        }
        return;
    case GGML_Q6_K:
        for (int64_t b = 0; b < n / 256; ++b, src += 210, out += 256) {
            const uint8_t *ql0 = src, *qh0 = src + 128;
            const int8_t* sc0 = reinterpret_cast<const int8_t*>(src + 192);
            const float d = half_to_f32(rd16(src + 208));
            for (int i = 0; i < 2; ++i) {
                const uint8_t *ql = ql0 + i * 64, *qh = qh0 + i * 32;
                const int8_t* sc = sc0 + i * 8;
                float* o = out + i * 128;
                for (int j = 0; j < 32; ++j) {
                    const int is = j / 16;
                    const int q0 = ((ql[j] & 0xF) | ((qh[j] & 0x03) << 4)) - 32;
                    const int q1 = ((ql[j + 32] & 0xF) | ((qh[j] & 0x0C) << 2)) - 32;
                    const int q2 = ((ql[j] >> 4) | (qh[j] & 0x30)) - 32;
                    const int q3 = ((ql[j + 32] >> 4) | ((qh[j] & 0xC0) >> 2)) - 32;
                    o[j] = d * (float)q0 * (float)sc[is];
                    o[j + 32] = d * (float)q1 * (float)sc[is + 2];
                    o[j + 64] = d * (float)q2 * (float)sc[is + 4];
                    o[j + 96] = d * (float)q3 * (float)sc[is + 6];
                }
            }
        }
        return;
    default:
        throw std::runtime_error(std::string("GGUF: cannot dequantize type ") + ggml_type_name(type));
    }
}

GgufFile::~GgufFile()
{
    if (map_) munmap(map_, size_);
}

void GgufFile::open(const std::string& path)
{
    path_ = path;
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("GGUF: cannot open " + path);
    struct stat st;
    if (fstat(fd, &st) != 0) {
        ::close(fd);
        throw std::runtime_error("GGUF: cannot stat " + path);
    }
    size_ = (size_t)st.st_size;
    if (size_ > 0) {
        map_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map_ == MAP_FAILED) {
            map_ = nullptr;
            ::close(fd);
            throw std::runtime_error("GGUF: cannot map " + path);
        }
    }
    ::close(fd);
    Reader r{static_cast<const uint8_t*>(map_), size_};
    const uint32_t magic = r.get<uint32_t>("magic");
    if (magic != 0x46554747u) throw std::runtime_error("GGUF: bad magic (not a GGUF file): " + path);
    const uint32_t version = r.get<uint32_t>("version");
    if (version != 3) throw std::runtime_error("GGUF: unsupported version " + std::to_string(version) + " (3 is)");
    const uint64_t n_tensors = r.get<uint64_t>("tensor count");
    const uint64_t n_kv = r.get<uint64_t>("metadata count");
    if (n_kv > size_ / 12) throw std::runtime_error("GGUF: metadata count " + std::to_string(n_kv) + " exceeds the file");
    if (n_tensors > size_ / 24) throw std::runtime_error("GGUF: tensor count " + std::to_string(n_tensors) + " exceeds the file");
    for (uint64_t i = 0; i < n_kv; ++i) {
        const std::string key = r.str("metadata key");
        const uint32_t t = r.get<uint32_t>("metadata type");
        Value v;
        v.type = t;
        switch (t) {
        case 0: v.u = r.get<uint8_t>("metadata value"); break;
        case 1: v.i = r.get<int8_t>("metadata value"); break;
        case 2: v.u = r.get<uint16_t>("metadata value"); break;
        case 3: v.i = r.get<int16_t>("metadata value"); break;
        case 4: v.u = r.get<uint32_t>("metadata value"); break;
        case 5: v.i = r.get<int32_t>("metadata value"); break;
        case 6: v.f = r.get<float>("metadata value"); break;
        case 7: v.u = r.get<uint8_t>("metadata value"); break;
        case 8: v.s = r.str("metadata string"); break;
        case 9: skip_value(r, 9, 0); break;
        case 10: v.u = r.get<uint64_t>("metadata value"); break;
        case 11: v.i = r.get<int64_t>("metadata value"); break;
        case 12: v.f = r.get<double>("metadata value"); break;
        default: throw std::runtime_error("GGUF: unknown metadata value type " + std::to_string(t) + " for key " + key);
        }
        if (t != 9) kv_[key] = v;
    }
    uint64_t alignment = 32;
    if (auto it = kv_.find("general.alignment"); it != kv_.end()) {
        alignment = it->second.type == 4 ? it->second.u : 0;
        if (alignment == 0 || (alignment & (alignment - 1)) || alignment > 65536)
            throw std::runtime_error("GGUF: invalid general.alignment");
    }
    struct Info {
        std::string name;
        uint32_t type;
        std::vector<int64_t> ne;
        uint64_t offset;
    };
    std::vector<Info> infos;
    for (uint64_t i = 0; i < n_tensors; ++i) {
        Info in;
        in.name = r.str("tensor name");
        const uint32_t nd = r.get<uint32_t>("tensor dims");
        if (nd == 0 || nd > 4) throw std::runtime_error("GGUF: tensor " + in.name + " has " + std::to_string(nd) + " dims");
        for (uint32_t k = 0; k < nd; ++k) {
            const uint64_t d = r.get<uint64_t>("tensor shape");
            if (d > (uint64_t)INT64_MAX) throw std::runtime_error("GGUF: tensor " + in.name + " dims overflow");
            in.ne.push_back((int64_t)d);
        }
        in.type = r.get<uint32_t>("tensor type");
        in.offset = r.get<uint64_t>("tensor offset");
        infos.push_back(std::move(in));
    }
    const uint64_t data_start = (r.pos + alignment - 1) / alignment * alignment;
    if (data_start > size_) throw std::runtime_error("GGUF: file is truncated (data section)");
    const size_t data_size = size_ - (size_t)data_start;
    for (Info& in : infos) {
        GgufTensor t;
        t.name = in.name;
        t.type = in.type;
        t.ne = in.ne;
        int64_t be = 0, bb = 0;
        int64_t numel = 1;
        for (int64_t d : in.ne)
            if (d != 0 && numel > INT64_MAX / d) throw std::runtime_error("GGUF: tensor " + in.name + " dims overflow");
            else numel *= d;
        if (ggml_block_geometry(in.type, &be, &bb)) {
            if (t.cols() % be != 0)
                throw std::runtime_error("GGUF: tensor " + in.name + " has " + std::to_string(t.cols()) + " columns, not a multiple of the " +
                                         ggml_type_name(in.type) + " block");
            const uint64_t blocks = (uint64_t)(numel / be);
            if (blocks > (uint64_t)data_size / (uint64_t)bb) throw std::runtime_error("GGUF: tensor " + in.name + " lies outside the file");
            t.nbytes = (size_t)(blocks * (uint64_t)bb);
            if (in.offset > data_size || t.nbytes > data_size - in.offset)
                throw std::runtime_error("GGUF: tensor " + in.name + " lies outside the file");
            t.data = static_cast<const uint8_t*>(map_) + data_start + in.offset;
        }
        // (a tensor of another type stays listed without data: using it raises an error that names the type)
        if (!tensors_.emplace(t.name, std::move(t)).second) throw std::runtime_error("GGUF: duplicate tensor " + in.name);
    }
    if (!get_string("general.architecture", &arch_)) arch_ = "llama";  // model_weights.rs:124
    uint32_t emb = 0, heads = 0;
    if (get_u32(arch_ + ".embedding_length", &emb) && get_u32(arch_ + ".attention.head_count", &heads) && heads > 0)
        head_dim_ = (int)(emb / heads);
}

bool GgufFile::get_u32(const std::string& key, uint32_t* out) const
{
    auto it = kv_.find(key);
    if (it == kv_.end()) return false;
    const Value& v = it->second;
    switch (v.type) {
    case 0: case 2: case 4: case 10:
        if (v.u > 0xFFFFFFFFull) return false;
        *out = (uint32_t)v.u;
        return true;
    case 1: case 3: case 5: case 11:
        if (v.i < 0 || v.i > 0xFFFFFFFFll) return false;
        *out = (uint32_t)v.i;
        return true;
    default: return false;
    }
}

bool GgufFile::get_f32(const std::string& key, float* out) const
{
    auto it = kv_.find(key);
    if (it == kv_.end() || (it->second.type != 6 && it->second.type != 12)) return false;
    *out = (float)it->second.f;
    return true;
}

bool GgufFile::get_string(const std::string& key, std::string* out) const
{
    auto it = kv_.find(key);
    if (it == kv_.end() || it->second.type != 8) return false;
    *out = it->second.s;
    return true;
}

const GgufTensor* GgufFile::find_hf(const std::string& hf_name) const
{
    auto it = tensors_.find(to_gguf_name(hf_name));
    return it == tensors_.end() ? nullptr : &it->second;
}

const GgufTensor& GgufFile::get_hf(const std::string& hf_name) const
{
    const GgufTensor* t = find_hf(hf_name);
    if (!t) throw std::runtime_error("GGUF: tensor " + to_gguf_name(hf_name) + " (" + hf_name + ") not found in " + path_);
    if (!t->data)
        throw std::runtime_error("GGUF: tensor " + t->name + " has unsupported type " + ggml_type_name(t->type) + " (" +
                                 std::to_string(t->type) + "); F32, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K and Q6_K are supported");
    return *t;
}

std::vector<uint8_t> GgufFile::rows_hf(const std::string& hf_name) const
{
    const GgufTensor& t = get_hf(hf_name);
    const int64_t rows = t.rows();
    const size_t row_bytes = rows ? t.nbytes / (size_t)rows : 0;
    std::vector<uint8_t> out(t.nbytes);
    const std::string g = t.name;
    const bool permuted = arch_ == "llama" && (ends_with(g, ".attn_q.weight") || ends_with(g, ".attn_k.weight"));
    if (!permuted) {
        if (t.nbytes) std::memcpy(out.data(), t.data, t.nbytes);
        return out;
    }
    const int64_t d = head_dim_;
    if (d <= 0 || (d & 1) || rows % d != 0) throw std::runtime_error("GGUF: tensor " + g + " rows do not divide into heads");
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t h = r / d, w = r % d;
        const int64_t src = h * d + (w < d / 2 ? 2 * w : 2 * (w - d / 2) + 1);
        std::memcpy(out.data() + (size_t)r * row_bytes, t.data + (size_t)src * row_bytes, row_bytes);
    }
    return out;
}

std::vector<int64_t> GgufFile::read_f32(const std::string& hf_name, std::vector<float>& out) const
{
    const GgufTensor& t = get_hf(hf_name);
    const std::vector<uint8_t> raw = rows_hf(hf_name);
    const int64_t rows = t.rows(), cols = t.cols();
    out.resize((size_t)(rows * cols));
    const size_t row_bytes = rows ? raw.size() / (size_t)rows : 0;
    for (int64_t r = 0; r < rows; ++r) ggml_dequantize_row(t.type, raw.data() + (size_t)r * row_bytes, cols, out.data() + (size_t)(r * cols));
    if (t.ne.size() == 1) return {cols};
    return {rows, cols};
}

std::string GgufFile::config_json() const
{
    const std::string& a = arch_;
    if (a == "qwen3moe")
        throw std::runtime_error("GGUF: unsupported architecture 'qwen3moe': quantized mixture-of-experts checkpoints (FP8, GGUF) are out of scope; "
                                 "qwen3_moe loads from bf16 or f32 safetensors");
    if (a != "llama" && a != "qwen2") throw std::runtime_error("GGUF: unsupported architecture '" + a + "' (llama and qwen2 are)");
    auto req = [&](const std::string& key) {
        uint32_t v = 0;
        if (!get_u32(key, &v)) throw std::runtime_error("GGUF: missing metadata key " + key);
        return v;
    };
    const uint32_t hidden = req(a + ".embedding_length"), inter = req(a + ".feed_forward_length"), heads = req(a + ".attention.head_count"),
                   layers = req(a + ".block_count"), ctx = req(a + ".context_length");
    uint32_t kv_heads = heads;
    (void)get_u32(a + ".attention.head_count_kv", &kv_heads);
    if (heads == 0 || hidden % heads != 0) throw std::runtime_error("GGUF: embedding_length is not a multiple of head_count");
    float theta = 10000.0f, eps = 1e-5f;
    (void)get_f32(a + ".rope.freq_base", &theta);
    (void)get_f32(a + ".attention.layer_norm_rms_epsilon", &eps);
    uint32_t bos = 128000, eos = 128001;
    (void)get_u32("tokenizer.ggml.bos_token_id", &bos);
    (void)get_u32("tokenizer.ggml.eos_token_id", &eos);
    const GgufTensor* emb = find_hf("model.embed_tokens.weight");
    if (!emb || emb->ne.size() != 2) throw std::runtime_error("GGUF: token_embd.weight is missing or not 2-D");
    const bool tied = find_hf("lm_head.weight") == nullptr;
    std::string j = "{";
    j += "\"architecture\": \"" + a + "\", \"model_type\": \"" + a + "\"";
    j += ", \"hidden_size\": " + std::to_string(hidden);
    j += ", \"intermediate_size\": " + std::to_string(inter);
    j += ", \"num_attention_heads\": " + std::to_string(heads);
    j += ", \"num_hidden_layers\": " + std::to_string(layers);
    j += ", \"num_key_value_heads\": " + std::to_string(kv_heads);
    j += ", \"head_dim\": " + std::to_string(hidden / heads);
    j += ", \"max_position_embeddings\": " + std::to_string(ctx);
    j += ", \"rope_theta\": " + fmt_float(theta);
    j += ", \"rms_norm_eps\": " + fmt_float(eps);
    j += ", \"vocab_size\": " + std::to_string(emb->ne[1]);
    j += ", \"bos_token_id\": " + std::to_string(bos);
    j += ", \"eos_token_id\": " + std::to_string(eos);
    j += std::string(", \"tie_word_embeddings\": ") + (tied ? "true" : "false");
    std::string rope_type;
    if (get_string(a + ".rope.scaling.type", &rope_type)) {
        float factor = 32.0f, low = 1.0f, high = 4.0f;
        uint32_t orig = 8192;
        (void)get_f32(a + ".rope.scaling.factor", &factor);
        (void)get_f32(a + ".rope.scaling.low_freq_factor", &low);
        (void)get_f32(a + ".rope.scaling.high_freq_factor", &high);
        (void)get_u32(a + ".rope.scaling.orig_ctx_len", &orig);
        j += ", \"rope_scaling\": {\"rope_type\": \"" + rope_type + "\", \"factor\": " + fmt_float(factor) +
             ", \"low_freq_factor\": " + fmt_float(low) + ", \"high_freq_factor\": " + fmt_float(high) +
             ", \"original_max_position_embeddings\": " + std::to_string(orig) + "}";
    } else {
        j += ", \"rope_scaling\": null";
    }
    j += "}";
    return j;
}

std::string resolve_gguf(const std::string& path)
{
    if (is_file(path)) return ends_with(path, ".gguf") ? path : std::string();
    if (!is_dir(path)) return std::string();
    if (is_file(path + "/model.safetensors") || is_file(path + "/model.safetensors.index.json")) return std::string();
    std::vector<std::string> names;
    if (DIR* d = opendir(path.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (ends_with(n, ".gguf") && is_file(path + "/" + n)) names.push_back(n);
        }
        closedir(d);
    }
    if (names.empty()) return std::string();
    std::sort(names.begin(), names.end());
    return path + "/" + names.front();
}

std::string checkpoint_dir(const std::string& path)
{
    if (is_dir(path)) return path;
    const size_t slash = path.rfind('/');
    return slash == std::string::npos ? std::string(".") : path.substr(0, slash);
}

}  // namespace kjarni
