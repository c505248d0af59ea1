// Read-only GGUF v3 view (mmap) for decoder checkpoints: the counterpart of GgufLoader + ModelWeights::from_gguf_file
// (crates/kjarni-transformers/src/weights/gguf_loader.rs, weights/model_weights.rs:45-170).
//
//   header      magic "GGUF", version 3, tensor count, metadata count; every metadata value type parses (arrays of
//               strings included), general.alignment (default 32) places the data section
//   tensors     name, ne[] (ne[0] = columns), ggml type, offset into the data section; F32 + Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 /
//               Q4_K / Q5_K / Q6_K matrices
//   names       HF names map to GGUF names as gguf_loader.rs:151-187 (+ blk.N.attn_{q,k,v}.bias for Qwen2)
//   Q/K rows    arch `llama`: llama.cpp's converter interleaved the rows of every head of attn_q / attn_k; rows() undoes it
//               per head_dim for every type (HF row r < d/2 <- GGUF row 2r, r >= d/2 <- 2(r - d/2) + 1)
//
// Every format problem (truncation, offsets outside the file, bad magic / version, overflowing dims, unsupported types)
// throws std::runtime_error with a message that names it; nothing reads outside the mapping.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace kjarni {

enum GgmlType : uint32_t {
    GGML_F32 = 0, GGML_F16 = 1, GGML_Q4_0 = 2, GGML_Q4_1 = 3, GGML_Q5_0 = 6, GGML_Q5_1 = 7, GGML_Q8_0 = 8, GGML_Q4_K = 12, GGML_Q5_K = 13,
    GGML_Q6_K = 14, GGML_BF16 = 30
};

const char* ggml_type_name(uint32_t type);
float f16_to_f32(uint16_t h);
void q4k_scale_min(int j, const uint8_t* scales, uint8_t* sc, uint8_t* m);  // get_scale_min_k4 (q_common.rs)
// Elements per block and bytes per block of a supported type (F32: 1 / 4); false for any other type.
bool ggml_block_geometry(uint32_t type, int64_t* elems, int64_t* bytes);
// Dequantizes n elements (n a multiple of the block size) of one row, with the reference's arithmetic
// (cpu/kernels/dequantize.rs:5-62).  Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K are unknown to the reference; the GGUF format defines
// them: w = (q - 8) d, q d + m, (q - 16) d, q d + m, (d sc) q - dmin m, each the f32 nearest to the exact value.
void ggml_dequantize_row(uint32_t type, const uint8_t* src, int64_t n, float* out);

struct GgufTensor {
    std::string name;
    uint32_t type = 0;
    std::vector<int64_t> ne;  // ne[0] = columns (fastest), ne[1] = rows
    const uint8_t* data = nullptr;
    size_t nbytes = 0;
    int64_t cols() const { return ne.empty() ? 1 : ne[0]; }
    int64_t rows() const
    {
        int64_t r = 1;
        for (size_t i = 1; i < ne.size(); ++i) r *= ne[i];
        return r;
    }
};

class GgufFile {
public:
    GgufFile() = default;
    ~GgufFile();
    GgufFile(const GgufFile&) = delete;
    GgufFile& operator=(const GgufFile&) = delete;

    void open(const std::string& path);
    const std::string& path() const { return path_; }
    const std::string& arch() const { return arch_; }

    // HF tensor name -> GGUF tensor (nullptr when absent)
    const GgufTensor* find_hf(const std::string& hf_name) const;
    const GgufTensor& get_hf(const std::string& hf_name) const;  // throws when absent
    // The tensor's rows in HF order (Q/K de-interleaved for arch llama), raw blocks: rows() x row_bytes
    std::vector<uint8_t> rows_hf(const std::string& hf_name) const;
    // Dequantized f32 in HF row order; returns {rows, cols} (or {n} for 1-D tensors)
    std::vector<int64_t> read_f32(const std::string& hf_name, std::vector<float>& out) const;
    // The decoder config synthesized from the metadata (model_weights.rs:123-170 + the choices in DESIGN.md)
    std::string config_json() const;
    int head_dim() const { return head_dim_; }
    const std::map<std::string, GgufTensor>& tensors() const { return tensors_; }

    bool get_u32(const std::string& key, uint32_t* out) const;
    bool get_f32(const std::string& key, float* out) const;
    bool get_string(const std::string& key, std::string* out) const;

private:
    struct Value {
        uint32_t type = 0;
        uint64_t u = 0;
        int64_t i = 0;
        double f = 0.0;
        std::string s;
    };
    std::string path_, arch_;
    void* map_ = nullptr;
    size_t size_ = 0;
    std::map<std::string, Value> kv_;  // scalars and strings (arrays are parsed and skipped)
    std::map<std::string, GgufTensor> tensors_;
    int head_dim_ = 0;
};

// A decoder checkpoint location as model_weights.rs:45-77 resolves it: a `.gguf` file, or a directory.  In a directory
// safetensors (model.safetensors / model.safetensors.index.json) win; otherwise the lexicographically first `*.gguf`.
// Returns the GGUF file to load, or "" when the location is a safetensors directory (or holds no GGUF).
std::string resolve_gguf(const std::string& path);
// The directory that holds the checkpoint: `path` itself, or the directory of a `.gguf` file.
std::string checkpoint_dir(const std::string& path);

}  // namespace kjarni
