#include "fp8_weights.h"

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "fp8_kernels.h"
#include "json.h"

namespace kjarni {

int fp8_scale_kind(int64_t n, int64_t k, int64_t scale_rows, int64_t scale_cols)
{
    if (scale_rows == 1 && scale_cols == 1) return FP8_PER_TENSOR;
    if (scale_rows == n && scale_cols == 1) return FP8_PER_CHANNEL;
    if (k % kFp8Block == 0 && scale_rows == (n + kFp8Block - 1) / kFp8Block && scale_cols == k / kFp8Block) return FP8_BLOCK;
    return -1;
}

float fp8_e4m3_to_f32(uint8_t code)
{
    const uint32_t sign = (uint32_t)(code & 0x80) << 24;
    const int exp = (code >> 3) & 0xF, man = code & 7;
    uint32_t bits;
    if (exp == 0xF && man == 7) {
        bits = sign | 0x7FC00000u;
    } else if (exp == 0) {
        float f = (float)man * 0.001953125f;  // subnormals: man / 8 * 2^-6
        std::memcpy(&bits, &f, 4);
        bits |= sign;
    } else {
        bits = sign | ((uint32_t)(exp - 7 + 127) << 23) | ((uint32_t)man << 20);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

namespace {

std::string shape_text(const std::vector<int64_t>& s)
{
    std::string t = "[";
    for (size_t i = 0; i < s.size(); ++i) t += (i ? ", " : "") + std::to_string(s[i]);
    return t + "]";
}

}  // namespace

Fp8Checkpoint::Fp8Checkpoint(const SafeTensors& st, const std::string& config_json) : st_(st)
{
    if (config_json.empty()) return;
    const Json cfg = Json::parse(config_json);
    const Json* q = cfg.find("quantization_config");
    if (!q || !q->is_object()) return;
    fmt_ = q->get_string("fmt", "");
    const Json* bs = q->find("weight_block_size");
    if (bs && bs->is_array())
        for (const Json& d : bs->arr) block_size_.push_back(d.as_int(-1));
}

bool Fp8Checkpoint::is_fp8(const std::string& name) const { return st_.contains(name) && st_.get(name).dtype == "F8_E4M3"; }

Fp8Tensor Fp8Checkpoint::read(const std::string& name) const
{
    const TensorView& w = st_.get(name);
    if (w.dtype != "F8_E4M3") throw std::runtime_error("tensor " + name + " is " + w.dtype + ", not F8_E4M3");
    if (!fmt_.empty() && fmt_ != "e4m3")
        throw std::runtime_error("FP8 tensor " + name + ": quantization_config.fmt is '" + fmt_ + "'; only e4m3 is supported");
    if (!block_size_.empty() && block_size_ != std::vector<int64_t>{kFp8Block, kFp8Block})
        throw std::runtime_error("FP8 tensor " + name + ": quantization_config.weight_block_size is " + shape_text(block_size_) +
                                 "; only [128, 128] is supported");
    if (w.shape.size() != 2 || w.shape[0] <= 0 || w.shape[1] <= 0)
        throw std::runtime_error("FP8 tensor " + name + " has shape " + shape_text(w.shape) + "; a matrix [n, k] is expected");
    Fp8Tensor t;
    t.n = w.shape[0];
    t.k = w.shape[1];
    if (w.nbytes != (size_t)(t.n * t.k)) throw std::runtime_error("size mismatch: " + name);
    if (t.k % 16) throw std::runtime_error("FP8 tensor " + name + " has k = " + std::to_string(t.k) + "; k % 16 == 0 is required");
    const std::string inv = name + "_scale_inv", plain = name + "_scale";
    const bool has_inv = st_.contains(inv), has_plain = st_.contains(plain);
    if (has_inv && has_plain) throw std::runtime_error("FP8 tensor " + name + " has both " + inv + " and " + plain + "; exactly one scale is expected");
    if (!has_inv && !has_plain) throw std::runtime_error("FP8 tensor " + name + " has no scale: neither " + inv + " nor " + plain + " is in the file");
    const std::string sname = has_inv ? inv : plain;
    const TensorView& sv = st_.get(sname);
    if (sv.dtype != "F32" && sv.dtype != "BF16" && sv.dtype != "F16")
        throw std::runtime_error("scale " + sname + " of FP8 tensor " + name + " has dtype " + sv.dtype + "; F32, BF16 or F16 is expected");
    const std::vector<int64_t>& ss = sv.shape;
    if (sv.numel() == 1 && ss.size() <= 2) {
        t.scale_rows = t.scale_cols = 1;
    } else if (ss.size() == 1) {
        t.scale_rows = ss[0];
        t.scale_cols = 1;
    } else if (ss.size() == 2) {
        t.scale_rows = ss[0];
        t.scale_cols = ss[1];
    }
    t.kind = ss.size() <= 2 && t.scale_rows > 0 ? fp8_scale_kind(t.n, t.k, t.scale_rows, t.scale_cols) : -1;
    if (t.kind < 0)
        throw std::runtime_error("scale " + sname + " of FP8 tensor " + name + " " + shape_text(w.shape) + " has shape " + shape_text(ss) +
                                 ": neither one element (per tensor), [n] / [n, 1] (per channel) nor [ceil(n / 128), k / 128] (block)");
    st_.read_f32(sname, t.scale);
    t.codes = w.data;
    for (int64_t i = 0, e = t.n * t.k; i < e; ++i)
        if ((t.codes[i] & 0x7F) == 0x7F) {
            char hex[8];
            std::snprintf(hex, sizeof hex, "0x%02X", t.codes[i]);
            throw std::runtime_error("FP8 tensor " + name + " holds a NaN code (" + hex + ") at row " + std::to_string(i / t.k) + ", column " +
                                     std::to_string(i % t.k));
        }
    return t;
}

std::vector<int64_t> Fp8Checkpoint::read_f32(const std::string& name, std::vector<float>& out) const
{
    const Fp8Tensor t = read(name);
    float table[256];
    for (int c = 0; c < 256; ++c) table[c] = fp8_e4m3_to_f32((uint8_t)c);
    out.resize((size_t)(t.n * t.k));
    const int shift = t.kind == FP8_BLOCK ? 7 : (t.kind == FP8_PER_CHANNEL ? 0 : 62);
    const int64_t col_mul = t.kind == FP8_BLOCK ? 1 : 0;
    for (int64_t j = 0; j < t.n; ++j) {
        const float* srow = t.scale.data() + (j >> shift) * t.scale_cols;
        const uint8_t* c = t.codes + j * t.k;
        float* o = out.data() + j * t.k;
        for (int64_t i = 0; i < t.k; ++i) o[i] = table[c[i]] * srow[(i >> 7) * col_mul];
    }
    return {t.n, t.k};
}

}  // namespace kjarni
