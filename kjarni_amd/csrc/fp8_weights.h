// FP8 (OCP e4m3fn) linear weights of a safetensors checkpoint, host side: `X.weight` of dtype F8_E4M3 beside exactly one scale
// tensor, `X.weight_scale_inv` (Qwen3's official -FP8 exports: 128 x 128 block scales) or `X.weight_scale` (compressed-tensors:
// per output channel or per tensor).  Both names mean w = decode(code) * scale.  Every refusal is a std::runtime_error that
// names the tensor and what was found.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "safetensors.h"

namespace kjarni {

// decode(code) of e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities; 0x7F / 0xFF are NaN; max 448.
float fp8_e4m3_to_f32(uint8_t code);

struct Fp8Tensor {
    int64_t n = 0, k = 0;
    const uint8_t* codes = nullptr;  // [n, k], a view into the mapped file
    std::vector<float> scale;        // widened to f32
    int64_t scale_rows = 0, scale_cols = 0;
    int kind = 0;  // FP8_PER_TENSOR / FP8_PER_CHANNEL / FP8_BLOCK (fp8_kernels.h)
};

class Fp8Checkpoint {
public:
    // config_json: the model's config.json ("" when there is none); its quantization_config is checked when a tensor is read
    // (fmt, when present, must be e4m3; weight_block_size, when present, must be [128, 128]).
    Fp8Checkpoint(const SafeTensors& st, const std::string& config_json);
    // `name` exists and holds F8_E4M3 codes
    bool is_fp8(const std::string& name) const;
    // The matrix `name` (X.weight) with its scale, checked: a missing scale, both scale names, a scale shape that fits no kind,
    // k % 16, a block size other than 128, another fmt, a NaN code.
    Fp8Tensor read(const std::string& name) const;
    // The same, dequantized: out[j, i] = decode(code) * scale in f32; returns the shape.
    std::vector<int64_t> read_f32(const std::string& name, std::vector<float>& out) const;

private:
    const SafeTensors& st_;
    std::string fmt_;                  // quantization_config.fmt ("" when absent)
    std::vector<int64_t> block_size_;  // quantization_config.weight_block_size (empty when absent)
};

}  // namespace kjarni
