// Token-level C ABI (include/kjarni_hip.h).
#include <cstring>
#include <memory>
#include <mutex>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "../../include/kjarni_hip.h"
#include "ffi_common.h"
#include "group.h"
#include "gguf.h"
#include "llm.h"
#include "decoder_embed_kernels.h"
#include "score_batch_kernels.h"
#include "answer_logits_kernels.h"
#include "llm_kernels.h"
#include "whisper_kernels.h"
#include "quant_kernels.h"
#include "moe_kernels.h"
#include "logprob_kernels.h"

using namespace kjarni;

struct KjarniHipEncoder {
    std::unique_ptr<EncoderModel> model;
};

namespace {

bool file_exists(const std::string& p)
{
    struct stat st;
    return ::stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// cpu/strategy.rs:43-44 (scratch buffers iff tokens <= 1 or tokens >= 1000) decides
// between the -inf (no-alloc) and -1e9 (alloc) mask fills on the embed path.
float resolve_fill(KjarniHipMaskFill fill, int64_t tokens, bool logits_path)
{
    const float neg_inf = -std::numeric_limits<float>::infinity();
    switch (fill) {
    case KJARNI_HIP_MASK_NEG_1E9: return -1e9f;
    case KJARNI_HIP_MASK_NEG_INF: return neg_inf;
    default: break;
    }
    if (logits_path) return -1e9f;  // forward_tokens: always encoder.forward (alloc path)
    return (tokens <= 1 || tokens >= 1000) ? neg_inf : -1e9f;
}

PoolMode pool_mode(KjarniHipPooling p)
{
    switch (p) {
    case KJARNI_HIP_POOL_MEAN: return POOL_MEAN;
    case KJARNI_HIP_POOL_CLS: return POOL_CLS;
    case KJARNI_HIP_POOL_MAX: return POOL_MAX;
    case KJARNI_HIP_POOL_LAST_TOKEN: return POOL_LAST;
    }
    throw InvalidConfig("unknown pooling strategy");
}

void check_shape(const EncoderModel& m, int64_t batch, int32_t seq)
{
    if (batch < 0 || seq < 0) throw InvalidConfig("negative batch or sequence length");
    if (seq > m.config().max_pos)
        throw InvalidConfig("sequence length " + std::to_string(seq) + " exceeds max_position_embeddings " +
                            std::to_string(m.config().max_pos));
}

struct DeviceBuf {
    void* p = nullptr;
    explicit DeviceBuf(size_t bytes) { hip_check(hipMalloc(&p, bytes ? bytes : 4), "hipMalloc"); }
    ~DeviceBuf()
    {
        if (p) (void)hipFree(p);
    }
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
};

void use_device(int32_t device)
{
    const int n = visible_device_count();
    if (n <= 0) throw GpuUnavailable("no HIP device is visible");
    if (device < 0 || device >= n) throw GpuUnavailable("HIP device index out of range");
    hip_check(hipSetDevice(device), "hipSetDevice");
}

}  // namespace

KJARNI_EXPORT int32_t kjarni_hip_device_count(void) { return visible_device_count(); }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_load(const char* model_dir, int32_t device,
                                                      KjarniHipEncoder** out)
{
    if (!model_dir || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        const std::string dir(model_dir);
        if (!file_exists(dir + "/config.json") ||
            !(file_exists(dir + "/model.safetensors") || file_exists(dir + "/model.safetensors.index.json")))
            throw ModelNotFound("model files not found in '" + dir +
                                "' (need config.json and model.safetensors)");
        auto h = std::make_unique<KjarniHipEncoder>();
        h->model = EncoderModel::load(dir, device);
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_encoder_free(KjarniHipEncoder* enc) { delete enc; }

KJARNI_EXPORT int32_t kjarni_hip_encoder_hidden_size(const KjarniHipEncoder* e) { return e ? e->model->config().hidden : 0; }
KJARNI_EXPORT int32_t kjarni_hip_encoder_num_layers(const KjarniHipEncoder* e) { return e ? e->model->config().layers : 0; }
KJARNI_EXPORT int32_t kjarni_hip_encoder_max_seq_len(const KjarniHipEncoder* e) { return e ? e->model->config().max_pos : 0; }
KJARNI_EXPORT int32_t kjarni_hip_encoder_vocab_size(const KjarniHipEncoder* e) { return e ? e->model->config().vocab : 0; }
KJARNI_EXPORT int32_t kjarni_hip_encoder_num_labels(const KjarniHipEncoder* e) { return e ? e->model->config().num_labels : 0; }
KJARNI_EXPORT int32_t kjarni_hip_encoder_device(const KjarniHipEncoder* e) { return e ? e->model->device() : -1; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_set_chunk_tokens(KjarniHipEncoder* enc, int64_t tokens)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    enc->model->set_chunk_tokens(tokens);
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_set_packing(KjarniHipEncoder* enc, int32_t on)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    enc->model->set_packing((int)on);
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_set_combining(KjarniHipEncoder* enc, int32_t on)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    enc->model->set_combining(on != 0);
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_set_two_lanes(KjarniHipEncoder* enc, int32_t on)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    enc->model->set_two_lanes(on != 0);
    return KJARNI_OK;
}

KJARNI_EXPORT int32_t kjarni_hip_set_f32_on_bf16(int32_t on)
{
    const int32_t before = kjarni::get_f32_on_bf16() ? 1 : 0;
    kjarni::set_f32_on_bf16(on != 0);
    return before;
}

KJARNI_EXPORT int32_t kjarni_hip_get_f32_on_bf16(void) { return kjarni::get_f32_on_bf16() ? 1 : 0; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_clock_probe(uint64_t* out_dev, uint32_t spin_us, void* stream)
{
    if (!out_dev) return KJARNI_ERROR_NULL_POINTER;
    const uint32_t us = spin_us == 0 ? 20u : (spin_us > 10000u ? 10000u : spin_us);
    return kjarni::launch_clock_probe(out_dev, us * 100u, (hipStream_t)stream) == hipSuccess ? KJARNI_OK
                                                                                             : KJARNI_ERROR_INFERENCE_FAILED;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_selftest_reductions(int32_t device, uint32_t waves, uint32_t seed, uint32_t* mismatches_out)
{
    if (!mismatches_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (waves == 0 || waves > (1u << 22)) throw InvalidConfig("1 .. 4 194 304 waves");
        use_device(device);
        DeviceBuf d(4);
        hip_check(hipMemset(d.p, 0, 4), "memset");
        hip_check(kjarni::launch_reduction_selftest((unsigned*)d.p, waves, seed, nullptr), "reduction self-test");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(mismatches_out, d.p, 4, hipMemcpyDeviceToHost), "D2H");
    });
}

namespace {
std::mutex g_measurement_mu;
constexpr int kMaxMeasurementDevices = 64;
hipStream_t g_measurement_stream[kMaxMeasurementDevices] = {};   // one per device, made on first use on that device
}  // namespace

KJARNI_EXPORT void* kjarni_hip_measurement_stream(void)
{
    // one non-blocking stream per DEVICE, made on first use with that device current (a measurement aid: see
    // kjarni_hip_clock_trace); a caller whose current device differs gets that device's own stream, never another's
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxMeasurementDevices) return nullptr;
    std::lock_guard<std::mutex> lock(g_measurement_mu);
    if (!g_measurement_stream[dev] && hipStreamCreateWithFlags(&g_measurement_stream[dev], hipStreamNonBlocking) != hipSuccess)
        g_measurement_stream[dev] = nullptr;
    return g_measurement_stream[dev];
}

KJARNI_EXPORT void kjarni_hip_measurement_stream_release(void)
{
    // (a process has a handful of hardware queues and HIP deals its streams over them: while this stream exists, one of the
    // encoder's own streams may share a queue with it -- a 64-sentence call, three parts on three streams, 1.72 -> 2.07 ms)
    std::lock_guard<std::mutex> lock(g_measurement_mu);
    int before = -1;
    (void)hipGetDevice(&before);
    for (int dev = 0; dev < kMaxMeasurementDevices; ++dev) {
        if (!g_measurement_stream[dev]) continue;
        (void)hipSetDevice(dev);
        (void)hipStreamSynchronize(g_measurement_stream[dev]);
        (void)hipStreamDestroy(g_measurement_stream[dev]);
        g_measurement_stream[dev] = nullptr;
    }
    if (before >= 0) (void)hipSetDevice(before);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_clock_trace(uint64_t* out_dev, uint32_t samples, uint32_t window_us, void* stream)
{
    if (!out_dev) return KJARNI_ERROR_NULL_POINTER;
    // (one launch stays below ten seconds: 1 .. 4096 windows of 10 us .. 1 s)
    if (samples == 0 || samples > 4096u || window_us < 10u || window_us > 1000000u || (uint64_t)samples * window_us > 10000000ull)
        return KJARNI_ERROR_INVALID_CONFIG;
    return kjarni::launch_clock_trace(out_dev, samples, window_us * 100u, (hipStream_t)stream) == hipSuccess ? KJARNI_OK
                                                                                                           : KJARNI_ERROR_INFERENCE_FAILED;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_hidden_states(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                                               const uint32_t* mask_dev,
                                                               const uint32_t* type_ids_dev, int64_t batch,
                                                               int32_t seq, KjarniHipMaskFill fill,
                                                               float* hidden_out_dev, void* stream)
{
    if (!enc || !ids_dev || !mask_dev || !hidden_out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->hidden_states(ids_dev, mask_dev, type_ids_dev, batch, seq,
                                  resolve_fill(fill, batch * seq, false), hidden_out_dev,
                                  static_cast<hipStream_t>(stream));
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_embed(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                                       const uint32_t* mask_dev, const uint32_t* type_ids_dev,
                                                       int64_t batch, int32_t seq, KjarniHipPooling pooling,
                                                       int32_t normalize, KjarniHipMaskFill fill,
                                                       float* out_dev, void* stream)
{
    if (!enc || !ids_dev || !mask_dev || !out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->embed(ids_dev, mask_dev, type_ids_dev, batch, seq, pool_mode(pooling), normalize != 0,
                          resolve_fill(fill, batch * seq, false), out_dev, static_cast<hipStream_t>(stream));
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_logits(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                                        const uint32_t* mask_dev, const uint32_t* type_ids_dev,
                                                        int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                                        float* logits_out_dev, void* stream)
{
    if (!enc || !ids_dev || !mask_dev || !logits_out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->logits(ids_dev, mask_dev, type_ids_dev, batch, seq, resolve_fill(fill, batch * seq, true),
                           logits_out_dev, static_cast<hipStream_t>(stream));
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_hidden_states_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                                                    const uint32_t* mask,
                                                                    const uint32_t* type_ids, int64_t batch,
                                                                    int32_t seq, KjarniHipMaskFill fill,
                                                                    float* hidden_out)
{
    if (!enc || !ids || !mask || !hidden_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->hidden_states_host(ids, mask, type_ids, batch, seq, resolve_fill(fill, batch * seq, false), hidden_out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_embed_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                                            const uint32_t* mask, const uint32_t* type_ids,
                                                            int64_t batch, int32_t seq, KjarniHipPooling pooling,
                                                            int32_t normalize, KjarniHipMaskFill fill, float* out)
{
    if (!enc || !ids || !mask || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->embed_host(ids, mask, type_ids, batch, seq, pool_mode(pooling), normalize != 0,
                               resolve_fill(fill, batch * seq, false), out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_logits_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                                             const uint32_t* mask, const uint32_t* type_ids,
                                                             int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                                             float* logits_out)
{
    if (!enc || !ids || !mask || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(*enc->model, batch, seq);
        enc->model->logits_host(ids, mask, type_ids, batch, seq, resolve_fill(fill, batch * seq, true), logits_out);
    });
}

// ---- several devices in one process (group.h) ----------------------------------------------------------

struct KjarniHipEncoderGroup {
    std::unique_ptr<EncoderGroup> group;
};

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_load(const char* model_dir, const int32_t* devices, size_t n_devices,
                                                    KjarniHipEncoderGroup** out)
{
    if (!model_dir || !out || (n_devices > 0 && !devices)) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        const std::string dir(model_dir);
        if (!file_exists(dir + "/config.json") ||
            !(file_exists(dir + "/model.safetensors") || file_exists(dir + "/model.safetensors.index.json")))
            throw ModelNotFound("model files not found in '" + dir + "' (need config.json and model.safetensors)");
        std::vector<int> devs(devices, devices + n_devices);
        if (devs.empty()) devs = devices_from_env();
        auto h = std::make_unique<KjarniHipEncoderGroup>();
        h->group = EncoderGroup::load(dir, devs);
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_group_free(KjarniHipEncoderGroup* g) { delete g; }
KJARNI_EXPORT size_t kjarni_hip_group_size(const KjarniHipEncoderGroup* g) { return g ? g->group->size() : 0; }
KJARNI_EXPORT int32_t kjarni_hip_group_device(const KjarniHipEncoderGroup* g, size_t i)
{
    return (g && i < g->group->size()) ? g->group->device(i) : -1;
}
KJARNI_EXPORT int32_t kjarni_hip_group_hidden_size(const KjarniHipEncoderGroup* g) { return g ? g->group->config().hidden : 0; }
KJARNI_EXPORT int32_t kjarni_hip_group_num_labels(const KjarniHipEncoderGroup* g) { return g ? g->group->config().num_labels : 0; }
KJARNI_EXPORT const char* kjarni_hip_group_transport(KjarniHipEncoderGroup* g)
{
    if (!g) return "";
    const char* t = "";
    (void)guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { t = g->group->transport(); });
    return t;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_shard(const KjarniHipEncoderGroup* g, int64_t rows, size_t i, int64_t* start_out,
                                                     int64_t* count_out)
{
    if (!g || !start_out || !count_out) return KJARNI_ERROR_NULL_POINTER;
    if (i >= g->group->size() || rows < 0) return KJARNI_ERROR_INVALID_CONFIG;
    EncoderGroup::shard(rows, g->group->size(), i, start_out, count_out);
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_gather_plan(int64_t rows, size_t n, int64_t width, KjarniHipGatherOp* ops_out, size_t cap,
                                                           size_t* count_out)
{
    if (!count_out || (cap && !ops_out)) return KJARNI_ERROR_NULL_POINTER;
    if (rows < 0 || n == 0 || n > 4096 || width <= 0) return KJARNI_ERROR_INVALID_CONFIG;
    const std::vector<EncoderGroup::GatherOp> plan = EncoderGroup::gather_plan(rows, n, width);
    *count_out = plan.size();
    for (size_t i = 0; i < plan.size() && i < cap; ++i) ops_out[i] = KjarniHipGatherOp{plan[i].rank, plan[i].root, plan[i].offset, plan[i].floats};
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_embed_host(KjarniHipEncoderGroup* g, const uint32_t* ids, const uint32_t* mask,
                                                          const uint32_t* type_ids, int64_t batch, int32_t seq,
                                                          KjarniHipPooling pooling, int32_t normalize, KjarniHipMaskFill fill,
                                                          float* out)
{
    if (!g || !ids || !mask || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(g->group->replica(0), batch, seq);
        g->group->embed_host(ids, mask, type_ids, batch, seq, pool_mode(pooling), normalize != 0,
                             resolve_fill(fill, batch * seq, false), out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_logits_host(KjarniHipEncoderGroup* g, const uint32_t* ids, const uint32_t* mask,
                                                           const uint32_t* type_ids, int64_t batch, int32_t seq,
                                                           KjarniHipMaskFill fill, float* logits_out)
{
    if (!g || !ids || !mask || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(g->group->replica(0), batch, seq);
        if (g->group->config().head_kind == 0) throw InvalidConfig("model has no classification head");
        g->group->logits_host(ids, mask, type_ids, batch, seq, resolve_fill(fill, batch * seq, true), logits_out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_embed_allgather(KjarniHipEncoderGroup* g, const uint32_t* const* ids_dev,
                                                               const uint32_t* const* mask_dev,
                                                               const uint32_t* const* type_ids_dev, int64_t batch_total,
                                                               int32_t seq, KjarniHipPooling pooling, int32_t normalize,
                                                               KjarniHipMaskFill fill, float* const* out_dev)
{
    if (!g || !ids_dev || !mask_dev || !out_dev) return KJARNI_ERROR_NULL_POINTER;
    for (size_t i = 0; i < g->group->size(); ++i)
        if (!ids_dev[i] || !mask_dev[i] || !out_dev[i]) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(g->group->replica(0), batch_total, seq);
        g->group->allgather_embed(ids_dev, mask_dev, type_ids_dev, batch_total, seq, pool_mode(pooling), normalize != 0,
                                  resolve_fill(fill, batch_total * seq, false), out_dev);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_group_logits_allgather(KjarniHipEncoderGroup* g, const uint32_t* const* ids_dev,
                                                                const uint32_t* const* mask_dev,
                                                                const uint32_t* const* type_ids_dev, int64_t batch_total,
                                                                int32_t seq, KjarniHipMaskFill fill, float* const* logits_out_dev)
{
    if (!g || !ids_dev || !mask_dev || !logits_out_dev) return KJARNI_ERROR_NULL_POINTER;
    for (size_t i = 0; i < g->group->size(); ++i)
        if (!ids_dev[i] || !mask_dev[i] || !logits_out_dev[i]) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_shape(g->group->replica(0), batch_total, seq);
        if (g->group->config().head_kind == 0) throw InvalidConfig("model has no classification head");
        g->group->allgather_logits(ids_dev, mask_dev, type_ids_dev, batch_total, seq, resolve_fill(fill, batch_total * seq, true),
                                   logits_out_dev);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_profile_begin(KjarniHipEncoder* enc)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { enc->model->profile_begin(); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_profile_begin_kinds(KjarniHipEncoder* enc, uint32_t kinds_mask)
{
    if (!enc) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { enc->model->profile_begin(kinds_mask); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_encoder_profile_end(KjarniHipEncoder* enc, KjarniHipKernelStat* stats_out,
                                                             size_t capacity, size_t* count_out)
{
    if (!enc || !stats_out || !count_out) return KJARNI_ERROR_NULL_POINTER;
    *count_out = 0;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const std::vector<KernelStat> st = enc->model->profile_end();
        size_t n = 0;
        for (const KernelStat& k : st) {
            if (n >= capacity) break;
            stats_out[n].kind = k.kind;
            stats_out[n].symbol = k.symbol;
            stats_out[n].launches = k.launches;
            stats_out[n].total_ms = k.total_ms;
            stats_out[n].flops = k.flops;
            stats_out[n].bytes = k.bytes;
            ++n;
        }
        *count_out = n;
    });
}

// ---- single operators -------------------------------------------------------------

namespace {

template <class F>
void time_launches(int32_t iters, float* ms_out, F&& launch)
{
    launch();  // the run whose result is returned
    if (iters > 0) {
        hipEvent_t a, b;
        hip_check(hipEventCreate(&a), "hipEventCreate");
        hip_check(hipEventCreate(&b), "hipEventCreate");
        hip_check(hipEventRecord(a, nullptr), "hipEventRecord");
        for (int32_t i = 0; i < iters; ++i) launch();
        hip_check(hipEventRecord(b, nullptr), "hipEventRecord");
        hip_check(hipEventSynchronize(b), "hipEventSynchronize");
        float ms = 0.0f;
        hip_check(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        if (ms_out) *ms_out = ms / (float)iters;
    }
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
}

// An output buffer with a guard band behind it: a kernel that writes past the end of its output writes here, silently
// otherwise.  check() reads the band back.
struct GuardedBuf {
    static constexpr uint32_t kGuard = 0x7fc0beefu;
    static constexpr size_t kGuardWords = 64;
    size_t bytes;
    DeviceBuf buf;
    explicit GuardedBuf(size_t b) : bytes((b + 3) / 4 * 4), buf(bytes + kGuardWords * 4)
    {
        hip_check(hipMemsetD32((hipDeviceptr_t)((char*)buf.p + bytes), (int)kGuard, kGuardWords), "guard band");
    }
    template <class T>
    T* as() const { return static_cast<T*>(buf.p); }
    void check(const char* what) const
    {
        uint32_t g[kGuardWords];
        hip_check(hipMemcpy(g, (char*)buf.p + bytes, sizeof(g), hipMemcpyDeviceToHost), "D2H guard band");
        for (size_t i = 0; i < kGuardWords; ++i)
            if (g[i] != kGuard) throw std::runtime_error(std::string(what) + ": guard band touched at word " + std::to_string(i));
    }
};

void expect(bool ok, const char* what)
{
    if (!ok) throw std::runtime_error(what);
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_linear(int32_t device, const float* x, const float* w, const float* bias,
                                                   const float* residual, int64_t m, int32_t k, int32_t n,
                                                   KjarniHipEpilogue epilogue, float* y, int32_t iters, float* ms_out)
{
    if (!x || !w || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || k <= 0 || n <= 0) throw InvalidConfig("invalid GEMM dimensions");
        if ((epilogue == KJARNI_HIP_EPI_BIAS_RESIDUAL || epilogue == KJARNI_HIP_EPI_BIAS_MUL_SILU) && !residual)
            throw InvalidConfig("residual epilogue without residual");
        use_device(device);
        if (m == 0) return;
        const size_t xb = (size_t)m * k * 4, wb = (size_t)n * k * 4, yb = (size_t)m * n * 4;
        // A guard band of one tile's rows behind the output: the tile kernels compute whole 128-row tiles and leave the rows past m
        // to a bounds check (a predicate, or the extent of a buffer descriptor) -- a wrong one would write here, silently.
        const size_t guard_floats = (size_t)128 * n;
        DeviceBuf xd(xb), wd(wb), bd((size_t)n * 4), rd(residual ? yb : 4), yd(yb + guard_floats * 4);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(wd.p, w, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, (size_t)n * 4, hipMemcpyHostToDevice), "H2D bias");
        if (residual) hip_check(hipMemcpy(rd.p, residual, yb, hipMemcpyHostToDevice), "H2D residual");
        constexpr uint32_t kGuard = 0x7fc0beefu;  // (a NaN no epilogue produces)
        hip_check(hipMemsetD32((hipDeviceptr_t)((char*)yd.p + yb), (int)kGuard, guard_floats), "guard band");
        // the scratch slab the encoder lends its GEMMs, so that the op takes the route the model takes at this row count
        const size_t sf = gemm_scratch_floats(m, n);
        DeviceBuf sd(sf * 4);
        const GemmScratch sc{(float*)sd.p, sf};
        time_launches(iters, ms_out, [&] {
            hip_check(launch_gemm((const float*)xd.p, k, (const float*)wd.p, bias ? (const float*)bd.p : nullptr,
                                  residual ? (const float*)rd.p : nullptr, n, (float*)yd.p, n, m, n, k,
                                  (GemmEpilogue)epilogue, nullptr, sc),
                      "gemm");
        });
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
        std::vector<uint32_t> guard(guard_floats);
        hip_check(hipMemcpy(guard.data(), (char*)yd.p + yb, guard_floats * 4, hipMemcpyDeviceToHost), "D2H guard band");
        for (size_t i = 0; i < guard_floats; ++i)
            if (guard[i] != kGuard) throw std::runtime_error("GEMM wrote past the last output row (guard band touched at float " + std::to_string(i) + ")");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_linear_bf16_weights(int32_t device, const float* x, const uint16_t* w_bf16,
                                                                const float* bias, const float* residual, int64_t m, int32_t k,
                                                                int32_t n, KjarniHipEpilogue epilogue, float* y, int32_t iters,
                                                                float* ms_out)
{
    if (!x || !w_bf16 || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || k <= 0 || n <= 0 || n % 128 != 0 || k % 64 != 0) throw InvalidConfig("invalid GEMM dimensions (n % 128, k % 64)");
        if ((epilogue == KJARNI_HIP_EPI_BIAS_RESIDUAL || epilogue == KJARNI_HIP_EPI_BIAS_MUL_SILU) && !residual)
            throw InvalidConfig("residual epilogue without residual");
        use_device(device);
        if (m == 0) return;
        const size_t xb = (size_t)m * k * 4, wb = (size_t)n * k * 2, yb = (size_t)m * n * 4;
        DeviceBuf xd(xb), wd(wb), bd((size_t)n * 4), rd(residual ? yb : 4), yd(yb);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(wd.p, w_bf16, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, (size_t)n * 4, hipMemcpyHostToDevice), "H2D bias");
        if (residual) hip_check(hipMemcpy(rd.p, residual, yb, hipMemcpyHostToDevice), "H2D residual");
        time_launches(iters, ms_out, [&] {
            hip_check(launch_gemm_bf16_weights((const float*)xd.p, k, wd.p, bias ? (const float*)bd.p : nullptr,
                                               residual ? (const float*)rd.p : nullptr, n, (float*)yd.p, n, m, n, k,
                                               (GemmEpilogue)epilogue, nullptr),
                      "gemm (bf16 weights)");
        });
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
    });
}

// The prompt-lookup draft kernel alone, on a history given by the host.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_lookup_draft(int32_t device, const uint32_t* tokens, size_t n, const KjarniHipLookupConfig* config,
                                                         uint32_t* draft_out, int32_t* n_out)
{
    if ((n && !tokens) || !draft_out || !n_out) return KJARNI_ERROR_NULL_POINTER;
    *n_out = 0;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        LookupConfig k;
        if (config) {
            k.draft_tokens = config->draft_tokens;
            k.ngram_max = config->ngram_max;
            k.ngram_min = config->ngram_min;
        }
        check_lookup_config(k);
        if (n > (size_t)std::numeric_limits<int32_t>::max()) throw InvalidConfig("history longer than 2^31 - 1 tokens");
        use_device(device);
        if (n == 0) return;
        DeviceBuf hist(n * sizeof(int32_t)), state(sizeof(LlmLookupState)), ids(8 * sizeof(uint32_t));
        LlmLookupState st = {};
        st.n = (int32_t)n;
        hip_check(hipMemcpy(hist.p, tokens, n * sizeof(int32_t), hipMemcpyHostToDevice), "H2D history");
        hip_check(hipMemcpy(state.p, &st, sizeof(st), hipMemcpyHostToDevice), "H2D state");
        hip_check(launch_lookup_draft(static_cast<const int32_t*>(hist.p), static_cast<LlmLookupState*>(state.p), k.ngram_max, k.ngram_min,
                                      k.draft_tokens, k.draft_tokens + 1, static_cast<uint32_t*>(ids.p), nullptr), "lookup draft");
        uint32_t rows[8] = {};
        hip_check(hipMemcpy(&st, state.p, sizeof(st), hipMemcpyDeviceToHost), "D2H state");
        hip_check(hipMemcpy(rows, ids.p, sizeof(rows), hipMemcpyDeviceToHost), "D2H ids");
        for (int i = 0; i < st.m; ++i) draft_out[i] = rows[1 + i];
        *n_out = st.m;
    });
}

// The shared-prefix copy kernel alone, on caches given by the host: src [2 * layers, src_floats] (K then V of each layer),
// dst [2 * layers, dst_floats] read and written back.  Every cache starts src_skew / dst_skew floats (0..3) past a 16-byte
// boundary, so a test reaches the 4-byte path; count floats go to dst_offset of every destination cache.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_kv_prefix_copy(int32_t device, const float* src, int32_t layers, int64_t src_floats, int32_t src_skew,
                                                           int64_t dst_floats, int32_t dst_skew, int64_t dst_offset, int64_t count, float* dst)
{
    if (!src || !dst) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (layers < 1 || layers > 1024 || src_floats < 1 || dst_floats < 1 || src_skew < 0 || src_skew > 3 || dst_skew < 0 || dst_skew > 3)
            throw InvalidConfig("invalid copy dimensions (layers 1..1024, floats >= 1, skews 0..3)");
        if (count < 0 || count > src_floats || dst_offset < 0 || dst_offset > dst_floats || count > dst_floats - dst_offset)
            throw InvalidConfig("count / dst_offset reach outside the caches");
        use_device(device);
        const size_t n = 2 * (size_t)layers;
        const size_t sstride = ((size_t)src_floats + 3 + 4) & ~(size_t)3, dstride = ((size_t)dst_floats + 3 + 4) & ~(size_t)3;  // 16-byte strides
        DeviceBuf sb(n * sstride * sizeof(float)), db(n * dstride * sizeof(float)), table((size_t)layers * sizeof(LlmKvCopyPair));
        std::vector<LlmKvCopyPair> pairs((size_t)layers);
        auto sp = [&](size_t i) { return static_cast<float*>(sb.p) + i * sstride + src_skew; };
        auto dp = [&](size_t i) { return static_cast<float*>(db.p) + i * dstride + dst_skew; };
        for (size_t i = 0; i < n; ++i) {
            hip_check(hipMemcpy(sp(i), src + i * (size_t)src_floats, (size_t)src_floats * sizeof(float), hipMemcpyHostToDevice), "H2D src");
            hip_check(hipMemcpy(dp(i), dst + i * (size_t)dst_floats, (size_t)dst_floats * sizeof(float), hipMemcpyHostToDevice), "H2D dst");
        }
        for (size_t l = 0; l < (size_t)layers; ++l) pairs[l] = {sp(2 * l), dp(2 * l), sp(2 * l + 1), dp(2 * l + 1)};
        hip_check(hipMemcpy(table.p, pairs.data(), pairs.size() * sizeof(LlmKvCopyPair), hipMemcpyHostToDevice), "H2D table");
        hip_check(launch_kv_prefix_copy(static_cast<const LlmKvCopyPair*>(table.p), layers, dst_offset, count, nullptr), "prefix copy");
        hip_check(hipDeviceSynchronize(), "sync");
        for (size_t i = 0; i < n; ++i)
            hip_check(hipMemcpy(dst + i * (size_t)dst_floats, dp(i), (size_t)dst_floats * sizeof(float), hipMemcpyDeviceToHost), "D2H dst");
    });
}

// Qwen3's per-head RMSNorm + RoPE kernel alone, on arrays given by the host: q [q_rows, ldq] and k [k_rows, ldk] are read,
// run through launch_qk_norm_rope for `rows` rows at base position `pos` (handed over in device memory when pos_on_device,
// as the captured step does) and written back whole, so a caller can check what the call left untouched.  cos_t / sin_t are
// [table_rows, head_dim / 2].
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_qk_norm_rope(int32_t device, float* q, int64_t ldq, int32_t q_rows, float* k, int64_t ldk,
                                                         int32_t k_rows, int32_t rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                                         const float* gamma_q, const float* gamma_k, float eps, const float* cos_t,
                                                         const float* sin_t, int32_t table_rows, int32_t pos, int32_t pos_on_device,
                                                         int32_t k_at_cache_row)
{
    if (!q || !k || !gamma_q || !gamma_k || !cos_t || !sin_t) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (head_dim < 2 || head_dim > 128 || (head_dim & 1) || n_heads < 1 || n_heads > 1024 || n_kv_heads < 1 || n_kv_heads > 1024)
            throw InvalidConfig("invalid head geometry (head_dim even, 2..128; heads and kv heads 1..1024)");
        if (rows < 1 || rows > q_rows || ldq < (int64_t)n_heads * head_dim || ldk < (int64_t)n_kv_heads * head_dim)
            throw InvalidConfig("rows / leading dimensions do not cover the heads");
        if (pos < 0 || table_rows < 1 || rows > table_rows - pos) throw InvalidConfig("positions reach outside the RoPE tables");
        if (k_at_cache_row ? (k_rows < 1 || rows > k_rows - pos) : rows > k_rows) throw InvalidConfig("K rows reach outside k");
        use_device(device);
        const size_t qb = (size_t)q_rows * (size_t)ldq * 4, kb = (size_t)k_rows * (size_t)ldk * 4, tb = (size_t)table_rows * (head_dim / 2) * 4;
        DeviceBuf qd(qb), kd(kb), gq((size_t)head_dim * 4), gk((size_t)head_dim * 4), cd(tb), sd(tb), pd(sizeof(int));
        hip_check(hipMemcpy(qd.p, q, qb, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, kb, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(gq.p, gamma_q, (size_t)head_dim * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(gk.p, gamma_k, (size_t)head_dim * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(cd.p, cos_t, tb, hipMemcpyHostToDevice), "H2D cos");
        hip_check(hipMemcpy(sd.p, sin_t, tb, hipMemcpyHostToDevice), "H2D sin");
        hip_check(hipMemcpy(pd.p, &pos, sizeof(int), hipMemcpyHostToDevice), "H2D pos");
        // (the device-held position wins inside the kernel: the host argument is then a value the result must not depend on)
        hip_check(launch_qk_norm_rope((float*)qd.p, ldq, (float*)kd.p, ldk, rows, n_heads, n_kv_heads, head_dim, (const float*)gq.p,
                                      (const float*)gk.p, eps, (const float*)cd.p, (const float*)sd.p, pos_on_device ? 0 : pos,
                                      pos_on_device ? (const int*)pd.p : nullptr, k_at_cache_row, nullptr), "qk norm + rope");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(q, qd.p, qb, hipMemcpyDeviceToHost), "D2H q");
        hip_check(hipMemcpy(k, kd.p, kb, hipMemcpyDeviceToHost), "D2H k");
    });
}

// ---- decoder embedders: the packed-row kernels alone ---------------------------------------------------------------------------

namespace {

// seq_start [n + 1]: starts at `first_min`..., strictly increasing, the last entry at most `rows`
void check_seq_start(const int32_t* seq_start, int32_t n, int32_t rows, bool from_zero)
{
    if (n < 1 || n > (1 << 20)) throw InvalidConfig("n_sequences must be 1 .. 2^20");
    if (from_zero ? seq_start[0] != 0 : seq_start[0] < 0) throw InvalidConfig(from_zero ? "seq_start[0] must be 0" : "seq_start[0] is negative");
    for (int32_t b = 0; b < n; ++b)
        if (seq_start[b + 1] <= seq_start[b])
            throw InvalidConfig("seq_start[" + std::to_string(b + 1) + "] does not exceed seq_start[" + std::to_string(b) + "]: sequence " +
                                std::to_string(b) + " is empty or the starts decrease");
    if (seq_start[n] > rows) throw InvalidConfig("seq_start[n_sequences] = " + std::to_string(seq_start[n]) + " reaches past the " +
                                                 std::to_string(rows) + " rows given");
}

void check_row_pos(const int32_t* row_pos, int32_t rows, int32_t table_rows)
{
    for (int32_t r = 0; r < rows; ++r)
        if (row_pos[r] < 0 || row_pos[r] >= table_rows)
            throw InvalidConfig("row_pos[" + std::to_string(r) + "] = " + std::to_string(row_pos[r]) + " is outside the RoPE tables");
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_packed_causal_attention(int32_t device, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                                    const float* v, int64_t ldv, int32_t buffer_rows, const int32_t* seq_start,
                                                                    int32_t n_sequences, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                                                    float* ctx, int64_t ldc)
{
    if (!q || !k || !v || !seq_start || !ctx) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) throw InvalidConfig("head_dim must be 16, 32, 64 or 128");
        if (heads < 1 || heads > 1024 || kv_heads < 1 || kv_heads > heads || heads % kv_heads)
            throw InvalidConfig("heads must be 1..1024 and a multiple of kv_heads");
        if (buffer_rows < 1 || buffer_rows > (1 << 22)) throw InvalidConfig("buffer_rows must be 1 .. 2^22");
        const int64_t qd = (int64_t)heads * head_dim, kvd = (int64_t)kv_heads * head_dim;
        if (ldq < qd || ldc < qd || ldk < kvd || ldv < kvd || ((ldq | ldk | ldv | ldc) & 3) || std::max(std::max(ldq, ldc), std::max(ldk, ldv)) > (1 << 20))
            throw InvalidConfig("leading dimensions must cover the heads, be multiples of 4 and at most 2^20");
        check_seq_start(seq_start, n_sequences, buffer_rows, true);
        std::vector<EmbedBlock> vec, mfma;
        for (int32_t b = 0; b < n_sequences; ++b) {
            const int32_t first = seq_start[b], len = seq_start[b + 1] - first;
            const bool m = embed_seq_takes_mfma(len, head_dim);
            for (int32_t q0 = 0; q0 < len; q0 += m ? 128 : 32) (m ? mfma : vec).push_back(EmbedBlock{first, q0, len});
        }
        use_device(device);
        const size_t R = (size_t)buffer_rows;
        DeviceBuf qd_(R * (size_t)ldq * 4), kd(R * (size_t)ldk * 4), vd(R * (size_t)ldv * 4), cd(R * (size_t)ldc * 4);
        DeviceBuf tv(vec.size() * sizeof(EmbedBlock)), tm(mfma.size() * sizeof(EmbedBlock));
        hip_check(hipMemcpy(qd_.p, q, R * (size_t)ldq * 4, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, R * (size_t)ldk * 4, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(vd.p, v, R * (size_t)ldv * 4, hipMemcpyHostToDevice), "H2D v");
        hip_check(hipMemcpy(cd.p, ctx, R * (size_t)ldc * 4, hipMemcpyHostToDevice), "H2D ctx");
        if (!vec.empty()) hip_check(hipMemcpy(tv.p, vec.data(), vec.size() * sizeof(EmbedBlock), hipMemcpyHostToDevice), "H2D blocks");
        if (!mfma.empty()) hip_check(hipMemcpy(tm.p, mfma.data(), mfma.size() * sizeof(EmbedBlock), hipMemcpyHostToDevice), "H2D blocks");
        hip_check(launch_packed_causal_attention((const float*)qd_.p, ldq, (const float*)kd.p, ldk, (const float*)vd.p, ldv,
                                                 (const EmbedBlock*)tv.p, (int)vec.size(), (const EmbedBlock*)tm.p, (int)mfma.size(), heads, head_dim,
                                                 heads / kv_heads, (float*)cd.p, ldc, nullptr), "packed attention");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(ctx, cd.p, R * (size_t)ldc * 4, hipMemcpyDeviceToHost), "D2H ctx");
    });
}

// ---- the decode attention and the projections that merge its slabs, alone ---------------------------------------------------------

namespace {

// A launcher's hipErrorInvalidValue is the caller's mistake, not a failed run.
void launcher_check(hipError_t e, const char* what)
{
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        throw InvalidConfig(std::string(what) + ": the launcher refuses these arguments");
    }
    hip_check(e, what);
}

size_t slab_floats(int32_t k, int32_t splits, int32_t head_dim) { return (size_t)(k / head_dim) * (size_t)splits * (size_t)(head_dim + 4); }

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_decode_attention(int32_t device, const float* q, int64_t ldq, int32_t rows, const float* k,
                                                             int64_t k_floats, int64_t ldk, const float* v, int64_t v_floats, int64_t ldv,
                                                             int32_t n_keys, int32_t keys_on_device, int32_t max_keys, int32_t heads,
                                                             int32_t head_dim, int32_t causal_base, int32_t splits, int32_t kv_group,
                                                             int64_t k_lane_stride, int64_t v_lane_stride, int32_t lanes,
                                                             const int32_t* lane_pos, const int32_t* lane_live, float* ctx, int64_t ldc,
                                                             float* slabs)
{
    if (!q || !k || !v || !ctx) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > 64 || heads < 1 || heads > 1024 || splits > 256 || kv_group < 1 || kv_group > heads)
            throw InvalidConfig("rows must be 1..64, heads 1..1024, splits at most 256, kv_group 1..heads");
        if (keys_on_device ? (n_keys < 0 || max_keys < 1 || max_keys > (1 << 20)) : (n_keys < 1 || n_keys > (1 << 20)))
            throw InvalidConfig("n_keys must be 1 .. 2^20 (with the count on the device: >= 0, and max_keys 1 .. 2^20)");
        if (!decode_attention_accepts(head_dim, splits, keys_on_device ? max_keys : n_keys, lanes, lane_pos != nullptr, lane_live != nullptr,
                                      keys_on_device != 0))
            throw InvalidConfig("launch_decode_attention refuses these arguments (head_dim a multiple of 4 dividing 1024, at most 128; splits "
                                ">= 1; at most 512 keys per split; ragged lanes need lanes, lane_live and the key count on the host)");
        if (lanes != 0 && lanes != rows) throw InvalidConfig("lanes must be 0 or rows");
        // every key row the kernel may touch lies inside the buffers given: the worst key count is what the form allows
        const int64_t keys = keys_on_device ? (int64_t)n_keys + (lanes ? 1 : rows) : n_keys;
        if (keys_on_device && keys > max_keys) throw InvalidConfig("the device count plus this step's rows exceeds max_keys");
        const int64_t qd = (int64_t)heads * head_dim, kvd = (int64_t)((heads - 1) / kv_group + 1) * head_dim;
        if (ldq < qd || ldc < qd || ldk < kvd || ldv < kvd || ((ldq | ldk | ldv | k_lane_stride | v_lane_stride) & 3) ||
            std::max(std::max(ldq, ldc), std::max(ldk, ldv)) > (1 << 20) || k_lane_stride < 0 || v_lane_stride < 0 ||
            std::max(k_lane_stride, v_lane_stride) > ((int64_t)1 << 28))
            throw InvalidConfig("leading dimensions must cover the heads, be multiples of 4 and at most 2^20; lane strides multiples of 4");
        if ((rows - 1) * k_lane_stride + (keys - 1) * ldk + kvd > k_floats || (rows - 1) * v_lane_stride + (keys - 1) * ldv + kvd > v_floats)
            throw InvalidConfig("the keys reach outside k_floats / v_floats");
        if (std::max(k_floats, v_floats) > ((int64_t)1 << 26)) throw InvalidConfig("k_floats / v_floats above 2^26");
        use_device(device);
        const size_t qb = (size_t)rows * (size_t)ldq * 4, cb = (size_t)rows * (size_t)ldc * 4;
        const size_t sb = decode_attention_scratch_floats(rows, heads, head_dim, splits) * 4;
        DeviceBuf qd_(qb), kd((size_t)k_floats * 4), vd((size_t)v_floats * 4), cd(cb), sd(sb), nd(sizeof(int)), pd((size_t)rows * 4), ld((size_t)rows * 4);
        hip_check(hipMemcpy(qd_.p, q, qb, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, (size_t)k_floats * 4, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(vd.p, v, (size_t)v_floats * 4, hipMemcpyHostToDevice), "H2D v");
        hip_check(hipMemcpy(cd.p, ctx, cb, hipMemcpyHostToDevice), "H2D ctx");
        hip_check(hipMemset(sd.p, 0xFF, sb), "poison scratch");  // (all-ones words are NaN: a slab the kernel skips would show)
        hip_check(hipMemcpy(nd.p, &n_keys, sizeof(int), hipMemcpyHostToDevice), "H2D n_keys");
        if (lane_pos) hip_check(hipMemcpy(pd.p, lane_pos, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D lane_pos");
        if (lane_live) hip_check(hipMemcpy(ld.p, lane_live, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D lane_live");
        // (with the count on the device the host's n_keys is a value the result must not depend on)
        launcher_check(launch_decode_attention((const float*)qd_.p, ldq, rows, (const float*)kd.p, ldk, (const float*)vd.p, ldv,
                                               keys_on_device ? 0 : n_keys, keys_on_device ? (const int*)nd.p : nullptr, max_keys, heads, head_dim,
                                               causal_base, splits, (float*)sd.p, (float*)cd.p, ldc, nullptr, kv_group, k_lane_stride,
                                               v_lane_stride, lanes, lane_pos ? (const int*)pd.p : nullptr,
                                               lane_live ? (const int*)ld.p : nullptr), "decode attention");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(ctx, cd.p, cb, hipMemcpyDeviceToHost), "D2H ctx");
        if (slabs) hip_check(hipMemcpy(slabs, sd.p, sb, hipMemcpyDeviceToHost), "D2H slabs");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_gemv_row_att(int32_t device, const float* slabs, int32_t splits, int32_t head_dim, const float* w,
                                                         const float* bias, const float* r, int32_t n_out, int32_t k, int32_t in_place,
                                                         int32_t two_step, float* y)
{
    if (!slabs || !w || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_out < 1 || n_out > 65536) throw InvalidConfig("n_out must be 1 .. 65536");
        if (!gemv_row_att_supported(k, splits, head_dim) || !r)
            throw InvalidConfig("launch_gemv_row_att refuses these arguments (k 512 or 2048, 1..16 splits, head_dim a multiple of 4 dividing k, "
                                "a residual)");
        use_device(device);
        const size_t sb = slab_floats(k, splits, head_dim) * 4, wb = (size_t)n_out * (size_t)k * 4, ob = (size_t)n_out * 4;
        DeviceBuf sd(sb), wd(wb), bd(ob), rd(ob), yd(ob), cd((size_t)k * 4);
        hip_check(hipMemcpy(sd.p, slabs, sb, hipMemcpyHostToDevice), "H2D slabs");
        hip_check(hipMemcpy(wd.p, w, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, ob, hipMemcpyHostToDevice), "H2D bias");
        hip_check(hipMemcpy(rd.p, r, ob, hipMemcpyHostToDevice), "H2D r");
        hip_check(hipMemset(yd.p, 0xFF, ob), "poison y");
        hip_check(hipMemset(cd.p, 0xFF, (size_t)k * 4), "poison ctx");
        float* out = in_place ? (float*)rd.p : (float*)yd.p;  // in place: the residual row is the output row, as in the decoder
        if (two_step) {  // the route the merging kernel replaces: combine, then the one-row projection + bias + residual
            launcher_check(launch_decode_attention_combine((const float*)sd.p, 1, k / head_dim, splits, head_dim, (float*)cd.p, k, nullptr),
                           "combine");
            GemvArgs a;
            a.X = (const float*)cd.p; a.ldx = k; a.rows = 1; a.W = (const float*)wd.p; a.bias = bias ? (const float*)bd.p : nullptr;
            a.R = (const float*)rd.p; a.ldr = n_out; a.n_out = n_out; a.k = k; a.Y0 = out; a.ldy0 = n_out; a.epi = EPI_BIAS_RESIDUAL;
            launcher_check(launch_gemv_rows(a, nullptr), "one-row projection");
        } else {
            launcher_check(launch_gemv_row_att((const float*)sd.p, splits, head_dim, (const float*)wd.p, bias ? (const float*)bd.p : nullptr,
                                               (const float*)rd.p, n_out, k, out, nullptr), "gemv_row_att");
        }
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(y, out, ob, hipMemcpyDeviceToHost), "D2H y");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_llm_gemv_att(int32_t device, const float* slabs, int32_t splits, int32_t head_dim, const void* w,
                                                         int32_t bf16, const float* bias, const float* r, int32_t n_out, int32_t k,
                                                         int32_t rows, float* y)
{
    if (!slabs || !w || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_out < 1 || n_out > 4096) throw InvalidConfig("n_out must be 1 .. 4096");
        if (rows != 1 || !llm_gemv_merges_attention(k, splits, head_dim) || !r)
            throw InvalidConfig("launch_llm_gemv refuses these arguments (one row; k 2048 with 1..8 splits or k 4096 with 1..4; head_dim a "
                                "multiple of 4 dividing k; a residual)");
        use_device(device);
        const size_t sb = slab_floats(k, splits, head_dim) * 4, wb = (size_t)n_out * (size_t)k * (bf16 ? 2 : 4), ob = (size_t)n_out * 4;
        DeviceBuf sd(sb), wd(wb), bd(ob), rd(ob), yd(ob);
        hip_check(hipMemcpy(sd.p, slabs, sb, hipMemcpyHostToDevice), "H2D slabs");
        hip_check(hipMemcpy(wd.p, w, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, ob, hipMemcpyHostToDevice), "H2D bias");
        hip_check(hipMemcpy(rd.p, r, ob, hipMemcpyHostToDevice), "H2D r");
        hip_check(hipMemset(yd.p, 0xFF, ob), "poison y");
        LlmGemvArgs a;
        a.X = (const float*)sd.p; a.ldx = k; a.rows = rows; a.W = wd.p; a.bf16 = bf16 ? 1 : 0; a.bias = bias ? (const float*)bd.p : nullptr;
        a.R = (const float*)rd.p; a.ldr = n_out; a.n_out = n_out; a.k = k; a.Y0 = (float*)yd.p; a.ldy0 = n_out;
        a.att_splits = splits; a.att_head_dim = head_dim;
        launcher_check(launch_llm_gemv(a, nullptr), "llm gemv + merge");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(y, yd.p, ob, hipMemcpyDeviceToHost), "D2H y");
    });
}

// ---- the prompt-route GEMM and the two prefill attention kernels, alone -----------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_prefill_gemm(int32_t device, const float* a, int64_t lda, int32_t a_rows, const void* w, int32_t bf16,
                                                         const float* bias, const float* r, int64_t ldr, int32_t r_is_y, float* y, int64_t ldy,
                                                         float* gate, int32_t m, int32_t n, int32_t k, int32_t split, int32_t* ksplit_used,
                                                         int64_t* scratch_written)
{
    if (!a || !w || !y || !ksplit_used) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || m > 4096 || a_rows < std::max(m, 1) || a_rows > 8192) throw InvalidConfig("m must be 0 .. 4096 and a_rows max(m, 1) .. 8192");
        if (n < 1 || k < 1 || n > (1 << 17) || k > (1 << 16) || (int64_t)n * k > ((int64_t)1 << 26))
            throw InvalidConfig("n must be 1 .. 2^17, k 1 .. 2^16, n * k at most 2^26");
        if (k % 32 || lda % 4) throw InvalidConfig("launch_prefill_gemm refuses these arguments: k a multiple of 32, lda a multiple of 4");
        if (lda < k || ldy < n || std::max(lda, ldy) > (1 << 18)) throw InvalidConfig("lda must cover k and ldy n (at most 2^18)");
        const bool res = r_is_y || r;
        const int64_t ldr_ = r_is_y ? ldy : ldr;  // in place the residual is the output: one stride, as rows_finish calls it
        if (res && (ldr_ < n || ldr_ > (1 << 18))) throw InvalidConfig("ldr must cover n (at most 2^18)");
        if (gate && (ldy != n || (n & 3))) throw InvalidConfig("launch_prefill_gemm refuses these arguments: a gate needs ldy == n and n a multiple of 4");
        if (split != 0 && split != 1) throw InvalidConfig("split must be 0 or 1");
        if (scratch_written && !split) throw InvalidConfig("scratch_written without split");
        use_device(device);
        const size_t ab = (size_t)a_rows * (size_t)lda * 4, wb = (size_t)n * (size_t)k * (bf16 ? 2 : 4), yb = (size_t)m * (size_t)ldy * 4;
        const size_t rb = r && !r_is_y ? (size_t)m * (size_t)ldr * 4 : 0, gb = gate ? (size_t)m * (size_t)n * 4 : 0;
        const size_t sb = split ? prefill_gemm_scratch_floats(m, n) * 4 : 0;
        DeviceBuf ad(ab), wd(wb), bd((size_t)n * 4), rd(rb), yd(yb), gd(gb), sd(sb);
        hip_check(hipMemcpy(ad.p, a, ab, hipMemcpyHostToDevice), "H2D a");
        hip_check(hipMemcpy(wd.p, w, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, (size_t)n * 4, hipMemcpyHostToDevice), "H2D bias");
        if (rb) hip_check(hipMemcpy(rd.p, r, rb, hipMemcpyHostToDevice), "H2D r");
        if (yb) hip_check(hipMemcpy(yd.p, y, yb, hipMemcpyHostToDevice), "H2D y");
        if (gb) hip_check(hipMemcpy(gd.p, gate, gb, hipMemcpyHostToDevice), "H2D gate");
        if (sb) hip_check(hipMemset(sd.p, 0xFF, sb), "poison scratch");  // (all-ones words are NaN: a slab the kernels skip would show)
        const float* bp = bias ? (const float*)bd.p : nullptr;
        const float* rp = r_is_y ? (const float*)yd.p : (r ? (const float*)rd.p : nullptr);
        float* sp = split ? (float*)sd.p : nullptr;
        *ksplit_used = prefill_gemm_launch_ksplit(bp, rp, ldr_, (const float*)yd.p, ldy, m, n, k, sp);
        launcher_check(launch_prefill_gemm((const float*)ad.p, lda, wd.p, bf16 ? 1 : 0, bp, rp, ldr_, (float*)yd.p, ldy, m, n, k, nullptr, sp,
                                           gate ? (float*)gd.p : nullptr), "prefill gemm");
        hip_check(hipDeviceSynchronize(), "sync");
        if (yb) hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
        if (gb) hip_check(hipMemcpy(gate, gd.p, gb, hipMemcpyDeviceToHost), "D2H gate");
        if (scratch_written) {  // the scratch words that no longer hold the poison
            std::vector<uint32_t> words(sb / 4);
            hip_check(hipMemcpy(words.data(), sd.p, sb, hipMemcpyDeviceToHost), "D2H scratch");
            *scratch_written = (int64_t)(words.size() - (size_t)std::count(words.begin(), words.end(), 0xFFFFFFFFu));
        }
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_prefill_attention(int32_t device, const float* q, int64_t ldq, int32_t rows, const float* k,
                                                              int64_t k_floats, int64_t ldk, const float* v, int64_t v_floats, int64_t ldv,
                                                              int32_t base, int32_t heads, int32_t head_dim, int32_t kv_group, float* ctx,
                                                              int64_t ldc, int32_t* route)
{
    if (!q || !k || !v || !ctx || !route) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (!prefill_attention_supported(head_dim)) throw InvalidConfig("launch_prefill_attention refuses these arguments: head_dim must be 16, 32, 64 or 128");
        if (rows < 1 || rows > 8192 || base < 0 || base > (1 << 20)) throw InvalidConfig("rows must be 1 .. 8192, base 0 .. 2^20");
        if (heads < 1 || heads > 1024 || kv_group < 1 || kv_group > heads || heads % kv_group)
            throw InvalidConfig("heads must be 1 .. 1024 and a multiple of kv_group");
        const int64_t qd = (int64_t)heads * head_dim, kvd = (int64_t)(heads / kv_group) * head_dim;
        if (ldq < qd || ldc < qd || ldk < kvd || ldv < kvd || ((ldq | ldk | ldv | ldc) & 3) || std::max(std::max(ldq, ldc), std::max(ldk, ldv)) > (1 << 20))
            throw InvalidConfig("leading dimensions must cover the heads, be multiples of 4 and at most 2^20");
        const int64_t keys = (int64_t)base + rows;
        if ((keys - 1) * ldk + kvd > k_floats || (keys - 1) * ldv + kvd > v_floats) throw InvalidConfig("the keys reach outside k_floats / v_floats");
        if (std::max(k_floats, v_floats) > ((int64_t)1 << 26)) throw InvalidConfig("k_floats / v_floats above 2^26");
        use_device(device);
        const size_t qb = (size_t)rows * (size_t)ldq * 4, cb = (size_t)rows * (size_t)ldc * 4;
        DeviceBuf qd_(qb), kd((size_t)k_floats * 4), vd((size_t)v_floats * 4), cd(cb);
        hip_check(hipMemcpy(qd_.p, q, qb, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, (size_t)k_floats * 4, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(vd.p, v, (size_t)v_floats * 4, hipMemcpyHostToDevice), "H2D v");
        hip_check(hipMemcpy(cd.p, ctx, cb, hipMemcpyHostToDevice), "H2D ctx");
        *route = prefill_attention_route((const float*)qd_.p, ldq, rows, (const float*)kd.p, ldk, (const float*)vd.p, ldv, head_dim);
        launcher_check(launch_prefill_attention((const float*)qd_.p, ldq, rows, (const float*)kd.p, ldk, (const float*)vd.p, ldv, base, heads,
                                                head_dim, kv_group, (float*)cd.p, ldc, nullptr), "prefill attention");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(ctx, cd.p, cb, hipMemcpyDeviceToHost), "D2H ctx");
    });
}

// ---- mixture-of-experts: the router pick and the sparse FFN, alone ------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_moe_route(int32_t device, const float* logits, int32_t rows, int32_t E, int32_t k, int32_t norm_topk,
                                                      int32_t* ids_out, float* weights_out)
{
    if (!logits || !ids_out || !weights_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (E < 2 || E > MOE_MAX_EXPERTS) throw InvalidConfig("E must be 2 .. 256");
        if (k < 1 || k > MOE_MAX_TOPK || k > E) throw InvalidConfig("k must be 1 .. 8 and at most E");
        if (rows < 1 || rows > (1 << 20)) throw InvalidConfig("rows must be 1 .. 2^20");
        use_device(device);
        const size_t lb = (size_t)rows * (size_t)E * 4, ob = (size_t)rows * (size_t)k * 4;
        DeviceBuf ld(lb), idd(ob), wd(ob);
        hip_check(hipMemcpy(ld.p, logits, lb, hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemset(idd.p, 0xFF, ob), "poison ids");
        hip_check(hipMemset(wd.p, 0xFF, ob), "poison weights");
        launcher_check(launch_moe_route((const float*)ld.p, E, rows, E, k, norm_topk ? 1 : 0, (int32_t*)idd.p, (float*)wd.p, nullptr), "moe route");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(ids_out, idd.p, ob, hipMemcpyDeviceToHost), "D2H ids");
        hip_check(hipMemcpy(weights_out, wd.p, ob, hipMemcpyDeviceToHost), "D2H weights");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_moe_ffn(int32_t device, const float* x, int64_t ldx, int32_t rows, const float* gamma, float eps,
                                                    const void* router, const void* gate, const void* up, const void* down, int32_t bf16,
                                                    int32_t hidden, int32_t E, int32_t k, int32_t Im, int32_t norm_topk, const float* r, int64_t ldr,
                                                    int32_t r_is_y, float* y, int64_t ldy, int32_t route, int32_t* ids_out, float* weights_out,
                                                    int32_t* route_used, int32_t* tiles_used)
{
    if (!x || !router || !gate || !up || !down || !y || !ids_out || !weights_out || !route_used || !tiles_used) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > 4096) throw InvalidConfig("rows must be 1 .. 4096");
        if (route < 0 || route > 2) throw InvalidConfig("route must be 0 (the decoders' rule), 1 (steps) or 2 (grouped)");
        if (!r_is_y && !r) throw InvalidConfig("a residual is needed: r, or r_is_y");
        const int64_t ldr_ = r_is_y ? ldy : ldr;
        MoeFfnArgs a;
        a.ldx = ldx; a.rows = rows; a.eps = eps; a.bf16 = bf16 ? 1 : 0; a.E = E; a.k = k; a.Im = Im; a.H = hidden; a.norm_topk = norm_topk ? 1 : 0;
        a.ldr = ldr_; a.ldy = ldy;
        MoeFfnArgs chk = a;
        chk.rows = 1;  // (the op runs the steps route in blocks of 8 rows and normalises a contiguous copy on the grouped route)
        chk.ldx = std::max<int64_t>(ldx, 0);
        if (const char* why = moe_ffn_refusal(chk, false)) throw InvalidConfig(std::string("the launchers refuse these arguments: ") + why);
        if (std::max(std::max(ldx, ldy), ldr_) > (1 << 18)) throw InvalidConfig("leading dimensions above 2^18");
        const int64_t stack = (int64_t)E * Im * hidden;
        if (stack > ((int64_t)1 << 27)) throw InvalidConfig("an expert stack above 2^27 elements");
        const bool grouped = route == 2 || (route == 0 && rows >= 24);
        use_device(device);
        const size_t wsz = bf16 ? 2 : 4, S = (size_t)rows * (size_t)k;
        const size_t xb = (size_t)rows * (size_t)ldx * 4, yb = (size_t)rows * (size_t)ldy * 4, rb = r_is_y ? 0 : (size_t)rows * (size_t)ldr * 4;
        DeviceBuf xd(xb), gd((size_t)hidden * 4), rtd((size_t)E * hidden * wsz), gtd((size_t)stack * wsz), upd((size_t)stack * wsz),
            dnd((size_t)stack * wsz), rd(rb), yd(yb), lg((size_t)rows * E * 4), idd(S * 4), wtd(S * 4), mid(S * (size_t)Im * 4);
        DeviceBuf xc(grouped && gamma ? (size_t)rows * hidden * 4 : 0), xn(grouped && gamma ? (size_t)rows * hidden * 4 : 0);
        DeviceBuf ys(grouped ? S * (size_t)hidden * 4 : 0), plan(grouped ? moe_plan_ints((int)S, E) * 4 : 0);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        if (gamma) hip_check(hipMemcpy(gd.p, gamma, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(rtd.p, router, (size_t)E * hidden * wsz, hipMemcpyHostToDevice), "H2D router");
        hip_check(hipMemcpy(gtd.p, gate, (size_t)stack * wsz, hipMemcpyHostToDevice), "H2D gate");
        hip_check(hipMemcpy(upd.p, up, (size_t)stack * wsz, hipMemcpyHostToDevice), "H2D up");
        hip_check(hipMemcpy(dnd.p, down, (size_t)stack * wsz, hipMemcpyHostToDevice), "H2D down");
        if (rb) hip_check(hipMemcpy(rd.p, r, rb, hipMemcpyHostToDevice), "H2D r");
        hip_check(hipMemcpy(yd.p, y, yb, hipMemcpyHostToDevice), "H2D y");
        hip_check(hipMemset(mid.p, 0xFF, S * (size_t)Im * 4), "poison mid");  // (all-ones words are NaN: a slot the kernels skip would show)
        hip_check(hipMemset(idd.p, 0xFF, S * 4), "poison ids");
        hip_check(hipMemset(wtd.p, 0xFF, S * 4), "poison weights");
        if (grouped) hip_check(hipMemset(ys.p, 0xFF, S * (size_t)hidden * 4), "poison y slots");
        a.gamma = gamma ? (const float*)gd.p : nullptr;
        a.router = rtd.p; a.gate = gtd.p; a.up = upd.p; a.down = dnd.p;
        *route_used = grouped ? 2 : 1;
        *tiles_used = 0;
        if (grouped) {
            a.X = (const float*)xd.p;
            if (gamma && ldx != hidden) {  // the norm kernel reads contiguous rows
                hip_check(hipMemcpy2D(xc.p, (size_t)hidden * 4, xd.p, (size_t)ldx * 4, (size_t)hidden * 4, (size_t)rows, hipMemcpyDeviceToDevice), "pack x");
                a.X = (const float*)xc.p;
                a.ldx = hidden;
            }
            a.xn = (float*)xn.p;
            a.R = r_is_y ? (const float*)yd.p : (const float*)rd.p; a.Y = (float*)yd.p;
            a.logits = (float*)lg.p; a.ids = (int32_t*)idd.p; a.weights = (float*)wtd.p; a.mid = (float*)mid.p; a.y = (float*)ys.p;
            a.plan = (int32_t*)plan.p;
            launcher_check(launch_moe_ffn_grouped(a, nullptr), "moe ffn (grouped)");
        } else {
            for (int r0 = 0; r0 < rows; r0 += 8) {
                MoeFfnArgs b = a;
                b.rows = std::min(8, rows - r0);
                b.X = (const float*)xd.p + (size_t)r0 * ldx;
                b.R = (r_is_y ? (const float*)yd.p : (const float*)rd.p) + (size_t)r0 * ldr_;
                b.Y = (float*)yd.p + (size_t)r0 * ldy;
                b.logits = (float*)lg.p + (size_t)r0 * E; b.ids = (int32_t*)idd.p + (size_t)r0 * k; b.weights = (float*)wtd.p + (size_t)r0 * k;
                b.mid = (float*)mid.p + (size_t)r0 * k * Im;
                launcher_check(launch_moe_ffn_steps(b, nullptr), "moe ffn (steps)");
            }
        }
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
        hip_check(hipMemcpy(ids_out, idd.p, S * 4, hipMemcpyDeviceToHost), "D2H ids");
        hip_check(hipMemcpy(weights_out, wtd.p, S * 4, hipMemcpyDeviceToHost), "D2H weights");
        if (grouped) hip_check(hipMemcpy(tiles_used, moe_plan_at((int32_t*)plan.p, (int)S, E).ntiles, 4, hipMemcpyDeviceToHost), "D2H tiles");
    });
}

namespace {

void rope_hook(int32_t device, float* x, int64_t ldx, int32_t x_rows, int32_t rows, int32_t n_heads, int32_t head_dim, const float* cos_t,
               const float* sin_t, int32_t table_rows, int32_t pos, const int32_t* row_pos)
{
    if (head_dim < 2 || head_dim > 256 || (head_dim & 1) || n_heads < 1 || n_heads > 1024)
        throw InvalidConfig("invalid head geometry (head_dim even, 2..256; heads 1..1024)");
    if (rows < 1 || rows > x_rows || x_rows > (1 << 22) || ldx < (int64_t)n_heads * head_dim || ldx > (1 << 20))
        throw InvalidConfig("rows / leading dimension do not cover the heads");
    if (table_rows < 1 || table_rows > (1 << 22)) throw InvalidConfig("table_rows must be 1 .. 2^22");
    if (row_pos) check_row_pos(row_pos, rows, table_rows);
    else if (pos < 0 || rows > table_rows - pos) throw InvalidConfig("positions reach outside the RoPE tables");
    use_device(device);
    const size_t xb = (size_t)x_rows * (size_t)ldx * 4, tb = (size_t)table_rows * (head_dim / 2) * 4;
    DeviceBuf xd(xb), cd(tb), sd(tb), pd((size_t)rows * 4);
    hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
    hip_check(hipMemcpy(cd.p, cos_t, tb, hipMemcpyHostToDevice), "H2D cos");
    hip_check(hipMemcpy(sd.p, sin_t, tb, hipMemcpyHostToDevice), "H2D sin");
    if (row_pos) {
        hip_check(hipMemcpy(pd.p, row_pos, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D row_pos");
        hip_check(launch_rope_rows((float*)xd.p, ldx, rows, n_heads, head_dim, (const float*)cd.p, (const float*)sd.p, (const int32_t*)pd.p, nullptr),
                  "rope rows");
    } else {
        hip_check(launch_rope((float*)xd.p, ldx, rows, n_heads, head_dim, (const float*)cd.p, (const float*)sd.p, pos, nullptr, 0, nullptr), "rope");
    }
    hip_check(hipDeviceSynchronize(), "sync");
    hip_check(hipMemcpy(x, xd.p, xb, hipMemcpyDeviceToHost), "D2H x");
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_rope(int32_t device, float* x, int64_t ldx, int32_t x_rows, int32_t rows, int32_t n_heads,
                                                 int32_t head_dim, const float* cos_t, const float* sin_t, int32_t table_rows, int32_t pos)
{
    if (!x || !cos_t || !sin_t) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { rope_hook(device, x, ldx, x_rows, rows, n_heads, head_dim, cos_t, sin_t, table_rows, pos, nullptr); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_rope_rows(int32_t device, float* x, int64_t ldx, int32_t x_rows, int32_t rows, int32_t n_heads,
                                                      int32_t head_dim, const float* cos_t, const float* sin_t, int32_t table_rows,
                                                      const int32_t* row_pos)
{
    if (!x || !cos_t || !sin_t || !row_pos) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { rope_hook(device, x, ldx, x_rows, rows, n_heads, head_dim, cos_t, sin_t, table_rows, 0, row_pos); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_qk_norm_rope_rows(int32_t device, float* q, int64_t ldq, int32_t q_rows, float* k, int64_t ldk,
                                                              int32_t k_rows, int32_t rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                                              const float* gamma_q, const float* gamma_k, float eps, const float* cos_t,
                                                              const float* sin_t, int32_t table_rows, const int32_t* row_pos)
{
    if (!q || !k || !gamma_q || !gamma_k || !cos_t || !sin_t || !row_pos) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (head_dim < 2 || head_dim > 128 || (head_dim & 1) || n_heads < 1 || n_heads > 1024 || n_kv_heads < 1 || n_kv_heads > 1024)
            throw InvalidConfig("invalid head geometry (head_dim even, 2..128; heads and kv heads 1..1024)");
        if (rows < 1 || rows > q_rows || rows > k_rows || q_rows > (1 << 22) || k_rows > (1 << 22) || ldq < (int64_t)n_heads * head_dim ||
            ldk < (int64_t)n_kv_heads * head_dim || ldq > (1 << 20) || ldk > (1 << 20))
            throw InvalidConfig("rows / leading dimensions do not cover the heads");
        if (table_rows < 1 || table_rows > (1 << 22)) throw InvalidConfig("table_rows must be 1 .. 2^22");
        check_row_pos(row_pos, rows, table_rows);
        use_device(device);
        const size_t qb = (size_t)q_rows * (size_t)ldq * 4, kb = (size_t)k_rows * (size_t)ldk * 4, tb = (size_t)table_rows * (head_dim / 2) * 4;
        DeviceBuf qd(qb), kd(kb), gq((size_t)head_dim * 4), gk((size_t)head_dim * 4), cd(tb), sd(tb), pd((size_t)rows * 4);
        hip_check(hipMemcpy(qd.p, q, qb, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, kb, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(gq.p, gamma_q, (size_t)head_dim * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(gk.p, gamma_k, (size_t)head_dim * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(cd.p, cos_t, tb, hipMemcpyHostToDevice), "H2D cos");
        hip_check(hipMemcpy(sd.p, sin_t, tb, hipMemcpyHostToDevice), "H2D sin");
        hip_check(hipMemcpy(pd.p, row_pos, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D row_pos");
        hip_check(launch_qk_norm_rope_rows((float*)qd.p, ldq, (float*)kd.p, ldk, rows, n_heads, n_kv_heads, head_dim, (const float*)gq.p,
                                           (const float*)gk.p, eps, (const float*)cd.p, (const float*)sd.p, (const int32_t*)pd.p, nullptr),
                  "qk norm + rope rows");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(q, qd.p, qb, hipMemcpyDeviceToHost), "D2H q");
        hip_check(hipMemcpy(k, kd.p, kb, hipMemcpyDeviceToHost), "D2H k");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_last_token_pool(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* seq_start,
                                                            int32_t n_sequences, int32_t hidden, const float* gamma, float eps, int32_t normalize,
                                                            float* out)
{
    if (!x || !seq_start || !gamma || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (hidden < 1 || hidden > 16384 || ldx < hidden || ldx > (1 << 20)) throw InvalidConfig("hidden must be 1 .. 16384 and ldx cover it");
        if (x_rows < 1 || x_rows > (1 << 22)) throw InvalidConfig("x_rows must be 1 .. 2^22");
        check_seq_start(seq_start, n_sequences, x_rows, false);
        use_device(device);
        const size_t xb = (size_t)x_rows * (size_t)ldx * 4, ob = (size_t)n_sequences * (size_t)hidden * 4;
        DeviceBuf xd(xb), gd((size_t)hidden * 4), sd(((size_t)n_sequences + 1) * 4);
        GuardedBuf od(ob);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(gd.p, gamma, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(sd.p, seq_start, ((size_t)n_sequences + 1) * 4, hipMemcpyHostToDevice), "H2D seq_start");
        hip_check(launch_last_token_pool((const float*)xd.p, ldx, (const int32_t*)sd.p, n_sequences, hidden, (const float*)gd.p, eps,
                                         normalize ? 1 : 0, od.as<float>(), nullptr), "last-token pool");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(out, od.buf.p, ob, hipMemcpyDeviceToHost), "D2H out");
        od.check("last-token pool");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_packed_prefix_attention(int32_t device, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                                    const float* v, int64_t ldv, int32_t buffer_rows, const int32_t* remainders,
                                                                    int32_t n_remainders, int32_t heads, int32_t kv_heads, int32_t head_dim,
                                                                    float* ctx, int64_t ldc)
{
    if (!q || !k || !v || !remainders || !ctx) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (head_dim != 16 && head_dim != 32 && head_dim != 64 && head_dim != 128) throw InvalidConfig("head_dim must be 16, 32, 64 or 128");
        if (heads < 1 || heads > 1024 || kv_heads < 1 || kv_heads > heads || heads % kv_heads)
            throw InvalidConfig("heads must be 1..1024 and a multiple of kv_heads");
        if (buffer_rows < 1 || buffer_rows > (1 << 22)) throw InvalidConfig("buffer_rows must be 1 .. 2^22");
        const int64_t qd = (int64_t)heads * head_dim, kvd = (int64_t)kv_heads * head_dim;
        if (ldq < qd || ldc < qd || ldk < kvd || ldv < kvd || ((ldq | ldk | ldv | ldc) & 3) || std::max(std::max(ldq, ldc), std::max(ldk, ldv)) > (1 << 20))
            throw InvalidConfig("leading dimensions must cover the heads, be multiples of 4 and at most 2^20");
        if (n_remainders < 1 || n_remainders > (1 << 20)) throw InvalidConfig("n_remainders must be 1 .. 2^20");
        std::vector<PrefixBlock> blocks;
        for (int32_t r = 0; r < n_remainders; ++r) {
            const int32_t first = remainders[4 * r], len = remainders[4 * r + 1], pf = remainders[4 * r + 2], pl = remainders[4 * r + 3];
            const std::string which = "remainders[" + std::to_string(r) + "]";
            if (first < 0 || len < 1 || len > buffer_rows - first)
                throw InvalidConfig(which + ": rows " + std::to_string(first) + " .. " + std::to_string((int64_t)first + len - 1) + " are outside the " +
                                    std::to_string(buffer_rows) + " rows given");
            if (pl < 0 || pf < 0 || pl > buffer_rows - pf)
                throw InvalidConfig(which + ": the prefix rows " + std::to_string(pf) + " .. " + std::to_string((int64_t)pf + pl - 1) +
                                    " are outside the " + std::to_string(buffer_rows) + " rows given");
            if (pl > 0 && pf < first + len && first < pf + pl) throw InvalidConfig(which + ": the prefix overlaps the remainder");
            for (int32_t q0 = 0; q0 < len; q0 += 32) blocks.push_back(PrefixBlock{first, q0, len, pf, pl});
        }
        use_device(device);
        const size_t R = (size_t)buffer_rows;
        DeviceBuf qd_(R * (size_t)ldq * 4), kd(R * (size_t)ldk * 4), vd(R * (size_t)ldv * 4), cd(R * (size_t)ldc * 4);
        DeviceBuf tb(blocks.size() * sizeof(PrefixBlock));
        hip_check(hipMemcpy(qd_.p, q, R * (size_t)ldq * 4, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.p, k, R * (size_t)ldk * 4, hipMemcpyHostToDevice), "H2D k");
        hip_check(hipMemcpy(vd.p, v, R * (size_t)ldv * 4, hipMemcpyHostToDevice), "H2D v");
        hip_check(hipMemcpy(cd.p, ctx, R * (size_t)ldc * 4, hipMemcpyHostToDevice), "H2D ctx");
        hip_check(hipMemcpy(tb.p, blocks.data(), blocks.size() * sizeof(PrefixBlock), hipMemcpyHostToDevice), "H2D blocks");
        hip_check(launch_packed_prefix_attention((const float*)qd_.p, ldq, (const float*)kd.p, ldk, (const float*)vd.p, ldv, (const PrefixBlock*)tb.p,
                                                 (int)blocks.size(), heads, head_dim, heads / kv_heads, (float*)cd.p, ldc, nullptr),
                  "packed prefix attention");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(ctx, cd.p, R * (size_t)ldc * 4, hipMemcpyDeviceToHost), "D2H ctx");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_score_gather_norm(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* src,
                                                              int32_t n, int32_t hidden, const float* gamma, const float* beta, float eps,
                                                              float* out, int64_t ldo)
{
    if (!x || !src || !gamma || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (hidden < 1 || hidden > 16384 || ldx < hidden || ldx > (1 << 20)) throw InvalidConfig("hidden must be 1 .. 16384 and ldx cover it");
        if (ldo < hidden || ldo > (1 << 20) || (ldo & 3)) throw InvalidConfig("ldo must cover hidden and be a multiple of 4");
        if (x_rows < 1 || x_rows > (1 << 22)) throw InvalidConfig("x_rows must be 1 .. 2^22");
        if (n < 1 || n > (1 << 20)) throw InvalidConfig("n must be 1 .. 2^20");
        for (int32_t j = 0; j < n; ++j)
            if (src[j] < 0 || src[j] >= x_rows)
                throw InvalidConfig("src[" + std::to_string(j) + "] = " + std::to_string(src[j]) + " is outside the " + std::to_string(x_rows) +
                                    " rows given");
        use_device(device);
        const size_t xb = (size_t)x_rows * (size_t)ldx * 4, ob = (size_t)n * (size_t)ldo * 4;
        DeviceBuf xd(xb), gd((size_t)hidden * 4), bd((size_t)hidden * 4), sd((size_t)n * 4);
        GuardedBuf od(ob);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(gd.p, gamma, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D gamma");
        if (beta) hip_check(hipMemcpy(bd.p, beta, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D beta");
        hip_check(hipMemcpy(sd.p, src, (size_t)n * 4, hipMemcpyHostToDevice), "H2D src");
        hip_check(hipMemcpy(od.buf.p, out, ob, hipMemcpyHostToDevice), "H2D out");  // (padding columns come back as given)
        hip_check(launch_score_gather_norm((const float*)xd.p, ldx, (const int32_t*)sd.p, n, hidden, (const float*)gd.p,
                                           beta ? (const float*)bd.p : nullptr, eps, od.as<float>(), ldo, nullptr), "score gather + norm");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(out, od.buf.p, ob, hipMemcpyDeviceToHost), "D2H out");
        od.check("score gather + norm");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_answer_logits(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* src, int32_t n,
                                                          int32_t hidden, const float* gamma, const float* beta, float eps, const void* head,
                                                          int32_t head_rows, int32_t head_is_bf16, const uint32_t* targets, int32_t n_targets,
                                                          float* out)
{
    if (!x || !src || !gamma || !head || !targets || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (hidden < 1 || hidden > 16384 || ldx < hidden || ldx > (1 << 20)) throw InvalidConfig("hidden must be 1 .. 16384 and ldx cover it");
        if (x_rows < 1 || x_rows > (1 << 22)) throw InvalidConfig("x_rows must be 1 .. 2^22");
        if (n < 1 || n > (1 << 20)) throw InvalidConfig("n must be 1 .. 2^20");
        if (head_rows < 1 || head_rows > (1 << 22)) throw InvalidConfig("head_rows must be 1 .. 2^22");
        if (n_targets < 1 || n_targets > kAnswerMaxTargets)
            throw InvalidConfig("n_targets (" + std::to_string(n_targets) + ") must be in [1, " + std::to_string(kAnswerMaxTargets) + "]");
        for (int32_t j = 0; j < n; ++j)
            if (src[j] < 0 || src[j] >= x_rows)
                throw InvalidConfig("src[" + std::to_string(j) + "] = " + std::to_string(src[j]) + " is outside the " + std::to_string(x_rows) +
                                    " rows given");
        for (int32_t t = 0; t < n_targets; ++t)
            if (targets[t] >= (uint32_t)head_rows)
                throw InvalidConfig("targets[" + std::to_string(t) + "] = " + std::to_string(targets[t]) + " is outside the " +
                                    std::to_string(head_rows) + " head rows given");
        use_device(device);
        const size_t xb = (size_t)x_rows * (size_t)ldx * 4, hb = (size_t)head_rows * (size_t)hidden * (head_is_bf16 ? 2 : 4);
        const size_t ob = (size_t)n * (size_t)n_targets * 4;
        DeviceBuf xd(xb), gd((size_t)hidden * 4), bd((size_t)hidden * 4), sd((size_t)n * 4), hd(hb), td((size_t)n_targets * 4);
        GuardedBuf od(ob);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(gd.p, gamma, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D gamma");
        if (beta) hip_check(hipMemcpy(bd.p, beta, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D beta");
        hip_check(hipMemcpy(sd.p, src, (size_t)n * 4, hipMemcpyHostToDevice), "H2D src");
        hip_check(hipMemcpy(hd.p, head, hb, hipMemcpyHostToDevice), "H2D head");
        hip_check(hipMemcpy(td.p, targets, (size_t)n_targets * 4, hipMemcpyHostToDevice), "H2D targets");
        hip_check(launch_answer_logits((const float*)xd.p, ldx, (const int32_t*)sd.p, n, hidden, (const float*)gd.p,
                                       beta ? (const float*)bd.p : nullptr, eps, hd.p, head_is_bf16 ? 1 : 0, (const uint32_t*)td.p, n_targets,
                                       od.as<float>(), nullptr), "answer logits");
        hip_check(hipDeviceSynchronize(), "sync");
        hip_check(hipMemcpy(out, od.buf.p, ob, hipMemcpyDeviceToHost), "D2H out");
        od.check("answer logits");
    });
}

// The greedy pick kernels alone, on logits given by the host: `calls` independent picks over logits [calls, rows, ld], each
// through the launcher the models use, on one scratch (which every call must leave zeroed for the next).
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_argmax(int32_t device, const float* logits, int32_t calls, int32_t rows, int64_t ld, int32_t vocab,
                                                   int32_t route, const int32_t* live, const uint32_t* draft, int32_t n_draft,
                                                   int32_t* picks_out, int32_t* accepted_out)
{
    if (!logits || !picks_out) return KJARNI_ERROR_NULL_POINTER;
    if (route == KJARNI_HIP_ARGMAX_LANES && !live) return KJARNI_ERROR_NULL_POINTER;
    if (route == KJARNI_HIP_ARGMAX_LOOKUP && ((n_draft > 0 && !draft) || !accepted_out)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (route < KJARNI_HIP_ARGMAX_DECODER || route > KJARNI_HIP_ARGMAX_LOOKUP) throw InvalidConfig("unknown argmax route");
        if (calls < 0 || vocab < 1 || ld < vocab) throw InvalidConfig("invalid argmax dimensions (calls >= 0, vocab >= 1, ld >= vocab)");
        if (rows < 1 || rows > kMaxLanes || (route == KJARNI_HIP_ARGMAX_DECODER && rows != 1))
            throw InvalidConfig("rows must be 1 (decoder route) or 1..8 (lanes, lookup)");
        if (route == KJARNI_HIP_ARGMAX_LOOKUP && (n_draft < 0 || n_draft > rows - 1)) throw InvalidConfig("n_draft must be 0..rows - 1");
        use_device(device);
        if (calls == 0) return;
        const size_t call_floats = (size_t)rows * (size_t)ld;
        DeviceBuf ld_buf((size_t)calls * call_floats * sizeof(float)), best(kMaxLanes * sizeof(unsigned long long));
        const float* dl = static_cast<const float*>(ld_buf.p);
        unsigned long long* dbest = static_cast<unsigned long long*>(best.p);
        hip_check(hipMemcpy(ld_buf.p, logits, (size_t)calls * call_floats * sizeof(float), hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemset(best.p, 0, kMaxLanes * sizeof(unsigned long long)), "memset");
        const auto best_is_zero = [&] {
            unsigned long long b[kMaxLanes];
            hip_check(hipMemcpy(b, best.p, sizeof(b), hipMemcpyDeviceToHost), "D2H best");
            for (int i = 0; i < kMaxLanes; ++i) expect(b[i] == 0ull, "the pick left its accumulator non-zero");
        };
        constexpr int32_t kUntouched = -77;

        if (route == KJARNI_HIP_ARGMAX_DECODER) {
            // as the replayed greedy step: the token is published, joins the history, count and position advance
            GuardedBuf out((size_t)calls * 4), hist((size_t)calls * 4);
            DeviceBuf counters(2 * sizeof(int));
            int* dc = static_cast<int*>(counters.p);
            hip_check(hipMemset(counters.p, 0, 2 * sizeof(int)), "memset");
            for (int32_t c = 0; c < calls; ++c)
                hip_check(launch_argmax(dl + (size_t)c * call_floats, vocab, dbest, out.as<int32_t>() + c, hist.as<int32_t>(), dc, dc + 1, nullptr),
                          "argmax");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            std::vector<int32_t> h((size_t)calls);
            int cnt[2] = {};
            hip_check(hipMemcpy(picks_out, out.buf.p, (size_t)calls * 4, hipMemcpyDeviceToHost), "D2H picks");
            hip_check(hipMemcpy(h.data(), hist.buf.p, (size_t)calls * 4, hipMemcpyDeviceToHost), "D2H history");
            hip_check(hipMemcpy(cnt, counters.p, sizeof(cnt), hipMemcpyDeviceToHost), "D2H counters");
            out.check("argmax token");
            hist.check("argmax history");
            best_is_zero();
            expect(cnt[0] == calls && cnt[1] == calls, "argmax: count / position did not advance by one per pick");
            for (int32_t c = 0; c < calls; ++c) expect(h[(size_t)c] == picks_out[c], "argmax: the history entry is not the pick");
            return;
        }

        if (route == KJARNI_HIP_ARGMAX_LANES) {
            constexpr int kStride = 4;
            GuardedBuf hist((size_t)kMaxLanes * kStride * 4), state(sizeof(LlmLaneState));
            LlmLaneState init = {};
            for (int l = 0; l < kMaxLanes; ++l) {
                init.token[l] = kUntouched - l;
                init.live[l] = l < rows && live[l] ? 1 : 0;
                init.limit[l] = 1 << 30;  // (no stop ids, a limit and a capacity no pick reaches: a live lane stays live)
            }
            std::vector<int32_t> h((size_t)kMaxLanes * kStride);
            for (int32_t c = 0; c < calls; ++c) {
                hip_check(hipMemcpy(state.buf.p, &init, sizeof(init), hipMemcpyHostToDevice), "H2D lane state");
                hip_check(hipMemsetD32((hipDeviceptr_t)hist.buf.p, kUntouched, (size_t)kMaxLanes * kStride), "memset history");
                hip_check(launch_lane_pick(dl + (size_t)c * call_floats, ld, vocab, rows, 0, dbest, state.as<LlmLaneState>(), hist.as<int32_t>(),
                                           kStride, 1 << 30, 1, nullptr), "lane pick");
                hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
                LlmLaneState st;
                hip_check(hipMemcpy(&st, state.buf.p, sizeof(st), hipMemcpyDeviceToHost), "D2H lane state");
                hip_check(hipMemcpy(h.data(), hist.buf.p, h.size() * 4, hipMemcpyDeviceToHost), "D2H history");
                hist.check("lane history");
                state.check("lane state");
                best_is_zero();
                for (int l = 0; l < kMaxLanes; ++l) {
                    const int32_t* hl = h.data() + (size_t)l * kStride;
                    if (init.live[l]) {
                        expect(st.live[l] == 1 && st.count[l] == 1 && st.pos[l] == 1, "lane pick: a live lane did not advance by one pick");
                        expect(hl[0] == st.token[l], "lane pick: the history entry is not the lane's next token");
                        for (int i = 1; i < kStride; ++i) expect(hl[i] == kUntouched, "lane pick: wrote past the lane's history entry");
                    } else {
                        expect(st.token[l] == init.token[l] && st.live[l] == 0 && st.count[l] == 0 && st.pos[l] == 0,
                               "lane pick: the state of a frozen lane changed");
                        for (int i = 0; i < kStride; ++i) expect(hl[i] == kUntouched, "lane pick: the history of a frozen lane changed");
                    }
                    if (l < rows) picks_out[(size_t)c * rows + l] = init.live[l] ? st.token[l] : -1;
                }
            }
            return;
        }

        // lookup: ids[0] = the last token, ids[1..n_draft] = the draft, the pad rows repeat the last of them (launch_lookup_draft)
        constexpr int kN0 = 5, kHistCap = kN0 + kMaxLanes;
        GuardedBuf hist((size_t)kHistCap * 4), state(sizeof(LlmLookupState)), log(2 * 4), pos(4);
        DeviceBuf ids(kMaxLanes * sizeof(uint32_t));
        std::vector<int32_t> h((size_t)kHistCap);
        for (int32_t c = 0; c < calls; ++c) {
            uint32_t row_ids[kMaxLanes] = {};
            for (int i = 1; i < kMaxLanes; ++i) row_ids[i] = i <= n_draft ? draft[(size_t)c * n_draft + (i - 1)] : row_ids[i - 1];
            LlmLookupState init = {};
            init.n = kN0;
            init.m = n_draft;
            for (int i = 0; i < 8; ++i) init.picks[i] = kUntouched;
            const int pos0 = kN0 - 1;
            hip_check(hipMemcpy(ids.p, row_ids, sizeof(row_ids), hipMemcpyHostToDevice), "H2D ids");
            hip_check(hipMemcpy(state.buf.p, &init, sizeof(init), hipMemcpyHostToDevice), "H2D lookup state");
            hip_check(hipMemcpy(pos.buf.p, &pos0, sizeof(pos0), hipMemcpyHostToDevice), "H2D pos");
            hip_check(hipMemsetD32((hipDeviceptr_t)hist.buf.p, kUntouched, (size_t)kHistCap), "memset history");
            hip_check(hipMemsetD32((hipDeviceptr_t)log.buf.p, kUntouched, 2), "memset log");
            hip_check(launch_lookup_pick(dl + (size_t)c * call_floats, ld, vocab, rows, static_cast<const uint32_t*>(ids.p), dbest,
                                         state.as<LlmLookupState>(), hist.as<int32_t>(), kHistCap, pos.as<int>(), log.as<int32_t>(), 1, nullptr),
                      "lookup pick");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            LlmLookupState st;
            int32_t lg[2] = {};
            int p1 = 0;
            hip_check(hipMemcpy(&st, state.buf.p, sizeof(st), hipMemcpyDeviceToHost), "D2H lookup state");
            hip_check(hipMemcpy(h.data(), hist.buf.p, h.size() * 4, hipMemcpyDeviceToHost), "D2H history");
            hip_check(hipMemcpy(lg, log.buf.p, sizeof(lg), hipMemcpyDeviceToHost), "D2H log");
            hip_check(hipMemcpy(&p1, pos.buf.p, sizeof(p1), hipMemcpyDeviceToHost), "D2H pos");
            hist.check("lookup history");
            state.check("lookup state");
            log.check("lookup log");
            pos.check("lookup position");
            best_is_zero();
            const int a = st.a;
            expect(a >= 0 && a <= n_draft, "lookup pick: accepted count outside 0..m");
            expect(st.n == kN0 + a + 1 && p1 == pos0 + a + 1 && st.steps == 1 && st.m == n_draft, "lookup pick: history length / position / steps");
            expect(lg[0] == n_draft && lg[1] == a, "lookup pick: the step log does not hold (m, a)");
            for (int i = 0; i < kHistCap; ++i) {
                const bool pick = i >= kN0 && i <= kN0 + a;
                expect(h[(size_t)i] == (pick ? st.picks[i - kN0] : kUntouched), "lookup pick: the history does not hold exactly the picks p_0..p_a");
            }
            for (int i = a + 1; i < 8; ++i) expect(st.picks[i] == kUntouched, "lookup pick: picks past p_a were written");
            for (int i = 0; i < rows; ++i) picks_out[(size_t)c * rows + i] = i <= a ? st.picks[i] : -1;
            accepted_out[c] = a;
        }
    });
}

// The logits processors alone: the history's counts built as LlmModel::generate builds them (one launch over the first n_bulk
// tokens -- the prompt --, one per later token), then the penalty and the n-gram ban over the whole history.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_logits_processors(int32_t device, const float* logits, int32_t vocab, const uint32_t* tokens, int32_t n,
                                                              int32_t n_bulk, float repetition_penalty, int32_t no_repeat_ngram, float* logits_out)
{
    if (!logits || !logits_out || (n > 0 && !tokens)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (vocab < 1 || n < 0 || n_bulk < 0 || n_bulk > n || no_repeat_ngram < 0)
            throw InvalidConfig("invalid logits-processor arguments (vocab >= 1, 0 <= n_bulk <= n, no_repeat_ngram >= 0)");
        use_device(device);
        GuardedBuf lg((size_t)vocab * 4), distinct((size_t)n * 4), counts((size_t)vocab * 4), nd(4);
        DeviceBuf tok((size_t)n * 4);
        hip_check(hipMemcpy(lg.buf.p, logits, (size_t)vocab * 4, hipMemcpyHostToDevice), "H2D logits");
        if (n) hip_check(hipMemcpy(tok.p, tokens, (size_t)n * 4, hipMemcpyHostToDevice), "H2D history");
        hip_check(hipMemset(counts.buf.p, 0, (size_t)vocab * 4), "memset counts");
        hip_check(hipMemset(nd.buf.p, 0, 4), "memset");
        const int32_t* dt = static_cast<const int32_t*>(tok.p);
        hip_check(launch_token_counts(dt, n_bulk, vocab, counts.as<int>(), distinct.as<int32_t>(), nd.as<int>(), nullptr), "token counts");
        for (int32_t i = n_bulk; i < n; ++i)
            hip_check(launch_token_counts(dt + i, 1, vocab, counts.as<int>(), distinct.as<int32_t>(), nd.as<int>(), nullptr), "token counts");
        hip_check(launch_logits_processors(lg.as<float>(), vocab, dt, n, counts.as<int>(), distinct.as<int32_t>(), nd.as<int>(), repetition_penalty,
                                           no_repeat_ngram, nullptr), "logits processors");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(logits_out, lg.buf.p, (size_t)vocab * 4, hipMemcpyDeviceToHost), "D2H logits");
        lg.check("processed logits");
        distinct.check("distinct tokens");
        counts.check("token counts");
        nd.check("distinct counter");
    });
}

// The sampler's cut alone: one launch_sample_candidates per row of logits (row c holds vocabs[c] floats, the rows packed one
// after another), in order, on ONE scratch and ONE header + candidate buffer as a generate call reuses them token after token.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_sample_candidates(int32_t device, const float* logits, const int32_t* vocabs, int32_t calls,
                                                              int64_t top_k, float top_p, float min_p, int32_t capacity,
                                                              KjarniHipSampleHeader* headers_out, uint32_t* ids_out, float* logits_out)
{
    if (!logits || !vocabs || !headers_out || !ids_out || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (calls < 0 || capacity < 1) throw InvalidConfig("invalid sampler arguments (calls >= 0, capacity >= 1)");
        size_t total = 0;
        for (int32_t c = 0; c < calls; ++c) {
            if (vocabs[c] < 1) throw InvalidConfig("vocabulary sizes must be positive");
            total += (size_t)vocabs[c];
        }
        use_device(device);
        if (calls == 0) return;
        DeviceBuf dl(total * 4), scratch(sample_scratch_bytes());
        GuardedBuf out(sizeof(SampleHeader) + (size_t)capacity * sizeof(SampleCandidate));
        hip_check(hipMemcpy(dl.p, logits, total * 4, hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemset(scratch.p, 0, sample_scratch_bytes()), "memset");
        hip_check(hipMemset(out.buf.p, 0, out.bytes), "memset");
        SampleHeader* dh = out.as<SampleHeader>();
        SampleCandidate* dc = reinterpret_cast<SampleCandidate*>(out.as<uint8_t>() + sizeof(SampleHeader));
        std::vector<SampleCandidate> cand((size_t)capacity);
        size_t off = 0;
        for (int32_t c = 0; c < calls; ++c) {
            hip_check(launch_sample_candidates(static_cast<const float*>(dl.p) + off, vocabs[c], top_k, top_p, min_p, scratch.p, dh, dc, capacity,
                                               nullptr), "sample candidates");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            off += (size_t)vocabs[c];
            SampleHeader h;
            hip_check(hipMemcpy(&h, dh, sizeof(h), hipMemcpyDeviceToHost), "D2H header");
            out.check("candidate list");
            const size_t n = std::min<size_t>(h.count, (size_t)capacity);
            if (n) hip_check(hipMemcpy(cand.data(), dc, n * sizeof(SampleCandidate), hipMemcpyDeviceToHost), "D2H candidates");
            headers_out[c] = KjarniHipSampleHeader{h.mx, h.sum, h.floor, h.count, h.overflow};
            for (size_t i = 0; i < n; ++i) {
                ids_out[(size_t)c * capacity + i] = cand[i].token;
                logits_out[(size_t)c * capacity + i] = cand[i].logit;
            }
        }
    });
}

// The rows cut alone: one launch_sample_candidates_rows over a block of logits rows.  The candidate slots start out as a
// sentinel: whatever a row does not own by its count must still hold it afterwards (a row that overflows writes nothing past
// its `capacity` slots, into no neighbour's list), and a guard band lies behind the scratch, the headers and the last list.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_sample_candidates_rows(int32_t device, const float* logits, int64_t ld, int32_t rows, int32_t vocab,
                                                                   int64_t top_k, float top_p, float min_p, int32_t capacity,
                                                                   KjarniHipSampleHeader* headers_out, uint32_t* ids_out, float* logits_out)
{
    if (!logits || !headers_out || !ids_out || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > 8 || vocab < 1 || ld < vocab || capacity < 1)
            throw InvalidConfig("invalid rows-sampler arguments (rows 1..8, vocab >= 1, ld >= vocab, capacity >= 1)");
        use_device(device);
        constexpr uint32_t kSentinel = 0xffffffffu;
        const size_t lbytes = (size_t)rows * (size_t)ld * 4, n_slots = sample_rows_entries(capacity);
        DeviceBuf dl(lbytes);
        GuardedBuf scratch(sample_scratch_rows_bytes(rows)), heads((size_t)rows * sizeof(SampleHeader)), cands(n_slots * sizeof(SampleCandidate));
        hip_check(hipMemcpy(dl.p, logits, lbytes, hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemset(scratch.buf.p, 0, scratch.bytes), "memset");
        hip_check(hipMemset(heads.buf.p, 0, heads.bytes), "memset");
        hip_check(hipMemset(cands.buf.p, 0xff, cands.bytes), "memset");
        hip_check(launch_sample_candidates_rows(static_cast<const float*>(dl.p), ld, rows, vocab, top_k, top_p, min_p, scratch.buf.p,
                                                heads.as<SampleHeader>(), cands.as<SampleCandidate>(), capacity, nullptr), "rows cut");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        std::vector<SampleHeader> h((size_t)rows);
        std::vector<SampleCandidate> c(n_slots);
        hip_check(hipMemcpy(h.data(), heads.buf.p, h.size() * sizeof(SampleHeader), hipMemcpyDeviceToHost), "D2H headers");
        hip_check(hipMemcpy(c.data(), cands.buf.p, c.size() * sizeof(SampleCandidate), hipMemcpyDeviceToHost), "D2H candidates");
        scratch.check("rows scratch");
        heads.check("rows headers");
        cands.check("rows candidates");
        std::vector<uint8_t> owned(n_slots, 0);
        for (int32_t r = 0; r < rows; ++r) {
            const SampleHeader& hr = h[(size_t)r];
            headers_out[r] = KjarniHipSampleHeader{hr.mx, hr.sum, hr.floor, hr.count, hr.overflow};
            const size_t own = hr.floor == -INFINITY ? 0 : std::min<size_t>(hr.count, (size_t)capacity);  // (no cut: nothing is appended)
            for (size_t i = 0; i < (size_t)capacity; ++i) {
                const size_t at = sample_rows_slot(r, (int)i);
                if (i < own) owned[at] = 1;
                ids_out[(size_t)r * capacity + i] = c[at].token;
                logits_out[(size_t)r * capacity + i] = c[at].logit;
            }
        }
        // every entry no row owns -- past a row's count, past its capacity, the rows that did not run -- still holds the sentinel
        for (size_t at = 0; at < n_slots; ++at) {
            uint32_t bits;
            std::memcpy(&bits, &c[at].logit, 4);
            if (!owned[at]) expect(c[at].token == kSentinel && bits == kSentinel, "rows cut: a slot that no row owns was written");
        }
    });
}

// The rows penalty alone: the counts of history[n_history] (it ends with ids[0]) built by launch_token_counts, then one
// launch_repetition_penalty_rows over logits [rows, ld].
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_repetition_penalty_rows(int32_t device, const float* logits, int64_t ld, int32_t rows, int32_t vocab,
                                                                    const uint32_t* ids, const uint32_t* history, int32_t n_history,
                                                                    float penalty, float* logits_out)
{
    if (!logits || !ids || !logits_out || (n_history > 0 && !history)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > 8 || vocab < 1 || ld < vocab || n_history < 0)
            throw InvalidConfig("invalid rows-penalty arguments (rows 1..8, vocab >= 1, ld >= vocab, n_history >= 0)");
        use_device(device);
        const size_t lbytes = (size_t)rows * (size_t)ld * 4;
        GuardedBuf lg(lbytes), distinct((size_t)n_history * 4), counts((size_t)vocab * 4), nd(4);
        DeviceBuf tok((size_t)n_history * 4), dids(8 * 4);
        hip_check(hipMemcpy(lg.buf.p, logits, lbytes, hipMemcpyHostToDevice), "H2D logits");
        if (n_history) hip_check(hipMemcpy(tok.p, history, (size_t)n_history * 4, hipMemcpyHostToDevice), "H2D history");
        hip_check(hipMemcpy(dids.p, ids, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D ids");
        hip_check(hipMemset(counts.buf.p, 0, (size_t)vocab * 4), "memset counts");
        hip_check(hipMemset(nd.buf.p, 0, 4), "memset");
        hip_check(launch_token_counts(static_cast<const int32_t*>(tok.p), n_history, vocab, counts.as<int>(), distinct.as<int32_t>(), nd.as<int>(),
                                      nullptr), "token counts");
        hip_check(launch_repetition_penalty_rows(lg.as<float>(), ld, rows, vocab, static_cast<const uint32_t*>(dids.p), counts.as<int>(),
                                                 distinct.as<int32_t>(), nd.as<int>(), penalty, nullptr), "rows penalty");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(logits_out, lg.buf.p, lbytes, hipMemcpyDeviceToHost), "D2H logits");
        lg.check("processed rows");
        distinct.check("distinct tokens");
        counts.check("token counts");
        nd.check("distinct counter");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_linear_ggml(int32_t device, const float* x, int64_t m, const void* blocks, int32_t ggml_type,
                                                        int32_t n, int32_t k, float* y)
{
    if (!x || !blocks || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        int64_t be = 0, bb = 0;
        if (!ggml_matrix_type((uint32_t)ggml_type) || !ggml_block_geometry((uint32_t)ggml_type, &be, &bb))
            throw InvalidConfig(std::string("unsupported GGML matrix type ") + ggml_type_name((uint32_t)ggml_type));
        if (m < 0 || n <= 0 || k <= 0 || k % 256 != 0) throw InvalidConfig("invalid quantized linear dimensions (k % 256)");
        use_device(device);
        if (m == 0) return;
        const QPlanes planes = repack_ggml((uint32_t)ggml_type, static_cast<const uint8_t*>(blocks), n, k);
        std::vector<std::unique_ptr<DeviceBuf>> pl;
        const void* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < 4; ++i) {
            if (planes.plane[i].empty()) continue;
            pl.push_back(std::make_unique<DeviceBuf>(planes.plane[i].size()));
            hip_check(hipMemcpy(pl.back()->p, planes.plane[i].data(), planes.plane[i].size(), hipMemcpyHostToDevice), "H2D weights");
            ptr[i] = pl.back()->p;
        }
        QMat W;
        W.type = (uint32_t)ggml_type; W.n = n; W.k = k; W.q = ptr[0]; W.q2 = ptr[1]; W.s = ptr[2]; W.s2 = ptr[3];
        const size_t xb = (size_t)m * k * 4, yb = (size_t)m * n * 4;
        DeviceBuf xd(xb), yd(yb);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        const float* X = static_cast<const float*>(xd.p);
        float* Y = static_cast<float*>(yd.p);
        if (m < 24) {  // the decoder's 8-row passes
            DeviceBuf codes((size_t)8 * k), scales((size_t)8 * (k / 256) * 4);
            for (int64_t r = 0; r < m; r += 8) {
                QGemvArgs a;
                a.W = W; a.X = X + r * k; a.ldx = k; a.rows = (int)std::min<int64_t>(8, m - r); a.Y = Y + r * n; a.ldy = n;
                if (W.type == GGML_Q6_K) {
                    hip_check(launch_q8k_quantize(a.X, k, a.rows, k, static_cast<int8_t*>(codes.p), static_cast<float*>(scales.p), nullptr, nullptr),
                              "q8k quantize");
                    a.Xq = static_cast<const int8_t*>(codes.p);
                    a.Xd = static_cast<const float*>(scales.p);
                }
                hip_check(launch_qgemv(a, nullptr), "quantized gemv");
            }
        } else {  // the prompt route: dequantized weights (+ Q8_K round trip of the activations for Q6_K) on the f32 matrix cores
            DeviceBuf w32((size_t)n * k * 4), xq(W.type == GGML_Q6_K ? xb : 4);
            hip_check(launch_qdequant(W, static_cast<float*>(w32.p), nullptr), "dequantize");
            if (W.type == GGML_Q6_K) {
                hip_check(launch_q8k_quantize(X, k, (int)m, k, nullptr, nullptr, static_cast<float*>(xq.p), nullptr), "q8k quantize");
                X = static_cast<const float*>(xq.p);
            }
            hip_check(launch_prefill_gemm(X, k, w32.p, 0, nullptr, nullptr, n, Y, n, (int)m, n, k, nullptr), "prefill gemm");
        }
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_linear_fp8(int32_t device, const float* x, int64_t m, const void* codes, const float* scale,
                                                       int32_t scale_rows, int32_t scale_cols, int32_t n, int32_t k, float* y)
{
    if (!x || !codes || !scale || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || n <= 0 || k <= 0 || k % 16 != 0) throw InvalidConfig("invalid FP8 linear dimensions (n, k >= 1, k % 16 == 0)");
        const int kind = fp8_scale_kind(n, k, scale_rows, scale_cols);
        if (kind < 0)
            throw InvalidConfig("FP8 linear: a scale of shape [" + std::to_string(scale_rows) + ", " + std::to_string(scale_cols) +
                                "] is neither [1, 1] (per tensor), [n, 1] (per channel) nor [ceil(n / 128), k / 128] (block)");
        const uint8_t* c = static_cast<const uint8_t*>(codes);
        for (int64_t i = 0, e = (int64_t)n * k; i < e; ++i)
            if ((c[i] & 0x7F) == 0x7F) throw InvalidConfig("FP8 linear: NaN code at element " + std::to_string(i));
        use_device(device);
        if (m == 0) return;
        const size_t wb = (size_t)n * k, sb = (size_t)scale_rows * scale_cols * 4, xb = (size_t)m * k * 4, yb = (size_t)m * n * 4;
        DeviceBuf wd(wb), sd(sb), xd(xb), yd(yb);
        hip_check(hipMemcpy(wd.p, codes, wb, hipMemcpyHostToDevice), "H2D codes");
        hip_check(hipMemcpy(sd.p, scale, sb, hipMemcpyHostToDevice), "H2D scales");
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        Fp8Mat W;
        W.n = n; W.k = k; W.codes = static_cast<const uint8_t*>(wd.p); W.scale = static_cast<const float*>(sd.p); W.kind = kind;
        const float* X = static_cast<const float*>(xd.p);
        float* Y = static_cast<float*>(yd.p);
        if (m < 24) {  // the decoder's 8-row passes
            for (int64_t r = 0; r < m; r += 8) {
                Fp8ProjArgs a;
                a.W[0] = W; a.X = X + r * k; a.ldx = k; a.rows = (int)std::min<int64_t>(8, m - r); a.Y[0] = Y + r * n; a.ldy[0] = n;
                hip_check(launch_fp8_proj(a, nullptr), "fp8 projection");
            }
        } else {  // the prompt route: dequantized weights on the f32 matrix cores
            DeviceBuf w32(wb * 4);
            hip_check(launch_fp8_dequant(W, static_cast<float*>(w32.p), nullptr), "dequantize");
            hip_check(launch_prefill_gemm(X, k, w32.p, 0, nullptr, nullptr, n, Y, n, (int)m, n, k, nullptr), "prefill gemm");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        }
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
    });
}

// ---- the decode step's fused projections and their preparation kernels, alone -----------------------------------------------------

namespace {

// What the two fused-projection entries share, checked before any GPU work: every element a kernel may read or write lies inside
// the buffers given.  n_mats / n_outs: matrices and output buffers of the mode.
struct ProjShape {
    int n_mats = 1, n_outs = 1;
    int64_t n_tot = 0;  // columns of the launch (SwiGLU: of one matrix)
};

ProjShape check_fused_proj(int32_t mode, const int32_t* n, int32_t k, int32_t rows_alloc, int64_t ldx, int32_t rows, const float* r, int64_t ldr,
                           int32_t r_is_y0, float* const* y, const int32_t* out_rows, const int64_t* ldy, int32_t row_off)
{
    if (mode < 0 || mode > 2) throw InvalidConfig("mode must be 0 (plain), 1 (Q | K | V) or 2 (SwiGLU)");
    ProjShape s;
    s.n_mats = mode == 1 ? 3 : (mode == 2 ? 2 : 1);
    s.n_outs = mode == 1 ? 3 : 1;
    if (k < 1 || k > (1 << 20)) throw InvalidConfig("k must be 1 .. 2^20");
    for (int i = 0; i < s.n_mats; ++i) {
        if (n[i] < 1 || n[i] > (1 << 20)) throw InvalidConfig("every matrix needs 1 .. 2^20 rows");
        s.n_tot += n[i];
    }
    if (mode == 2) {
        if (n[1] != n[0]) throw InvalidConfig("gate and up must have the same number of rows");
        s.n_tot = n[0];
    }
    if (rows < 0 || rows > 64 || rows_alloc < 1 || rows > rows_alloc || rows_alloc > 64) throw InvalidConfig("rows must be 0 .. rows_alloc <= 64");
    if (ldx < k || ldx > (1 << 21) || (ldx & 3)) throw InvalidConfig("ldx must cover k, be a multiple of 4 and at most 2^21");
    if (row_off < 0) throw InvalidConfig("row_off must not be negative");
    for (int i = 0; i < s.n_outs; ++i) {
        if (!y[i]) throw InvalidConfig("an output of this mode is NULL");
        const int64_t cols = mode == 2 ? n[0] : n[i];
        if (ldy[i] < cols || ldy[i] > (1 << 21) || out_rows[i] < 1 || out_rows[i] > 4096) throw InvalidConfig("ldy must cover the matrix's rows; out_rows 1 .. 4096");
        if ((int64_t)(i == 0 ? 0 : row_off) + rows > out_rows[i])
            throw InvalidConfig("rows " + std::to_string(i == 0 ? 0 : row_off) + " .. +" + std::to_string(rows) + " do not fit the " +
                                std::to_string(out_rows[i]) + " rows of output " + std::to_string(i));
    }
    if (r && r_is_y0) throw InvalidConfig("r_is_y0 takes the residual from y[0]: r must be NULL");
    if ((r || r_is_y0) && mode == 1) throw InvalidConfig("no residual with Q | K | V: its columns span three outputs");
    if (r && (ldr < s.n_tot || ldr > (1 << 21))) throw InvalidConfig("ldr must cover the columns");
    return s;
}

// The output buffers of a fused projection on the device: uploaded whole, a guard band behind each, downloaded whole.
struct ProjOutputs {
    std::vector<std::unique_ptr<GuardedBuf>> buf;
    std::vector<size_t> bytes;
    ProjOutputs(const ProjShape& s, float* const* y, const int32_t* out_rows, const int64_t* ldy)
    {
        for (int i = 0; i < s.n_outs; ++i) {
            bytes.push_back((size_t)out_rows[i] * (size_t)ldy[i] * 4);
            buf.push_back(std::make_unique<GuardedBuf>(bytes.back()));
            hip_check(hipMemcpy(buf.back()->buf.p, y[i], bytes.back(), hipMemcpyHostToDevice), "H2D y");
        }
    }
    float* dev(int i) const { return i < (int)buf.size() ? buf[i]->as<float>() : nullptr; }
    void fetch(float* const* y) const
    {
        for (size_t i = 0; i < buf.size(); ++i) {
            buf[i]->check("fused projection output");
            hip_check(hipMemcpy(y[i], buf[i]->buf.p, bytes[i], hipMemcpyDeviceToHost), "D2H y");
        }
    }
};

// With the offset on the device the launcher's row_off is a value the result must not depend on: another row that is still inside
// every buffer (`room` = the largest offset all of them allow), so that a kernel reading the wrong one writes a wrong row, not
// outside.
int decoy_offset(int32_t row_off, int64_t room) { return row_off != 0 ? 0 : (int)std::max<int64_t>(room, 0); }

std::unique_ptr<DeviceBuf> upload(const void* src, size_t bytes, const char* what)
{
    auto d = std::make_unique<DeviceBuf>(bytes);
    if (src && bytes) hip_check(hipMemcpy(d->p, src, bytes, hipMemcpyHostToDevice), what);
    return d;
}

// Raw GGUF blocks [n, k] of one type -> the device planes of a QMat (kept alive by `keep`).
// (a Q8_0 matrix with k % 256 != 0 can be repacked: it is the launcher that refuses it)
void check_qmat_type(int32_t ggml_type, int32_t k)
{
    if (!ggml_matrix_type((uint32_t)ggml_type)) throw InvalidConfig(std::string("unsupported GGML matrix type ") + ggml_type_name((uint32_t)ggml_type));
    if (k % 32 || (ggml_type != (int32_t)GGML_Q8_0 && k % 256)) throw InvalidConfig("k must be a whole number of the type's blocks");
}

QMat upload_qmat(int32_t ggml_type, const void* blocks, int32_t n, int32_t k, std::vector<std::unique_ptr<DeviceBuf>>& keep)
{
    const QPlanes planes = repack_ggml((uint32_t)ggml_type, static_cast<const uint8_t*>(blocks), n, k);
    const void* ptr[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        if (planes.plane[i].empty()) continue;
        keep.push_back(upload(planes.plane[i].data(), planes.plane[i].size(), "H2D weights"));
        ptr[i] = keep.back()->p;
    }
    QMat W;
    W.type = (uint32_t)ggml_type; W.n = n; W.k = k; W.q = ptr[0]; W.q2 = ptr[1]; W.s = ptr[2]; W.s2 = ptr[3];
    return W;
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_fused_proj_fp8(int32_t device, int32_t mode, const void* const* codes, const float* const* scales,
                                                           const int32_t* scale_rows, const int32_t* scale_cols, const int32_t* n, int32_t k,
                                                           const float* x, int32_t rows_alloc, int64_t ldx, int32_t rows, const float* gamma,
                                                           float eps, const float* bias, const float* r, int64_t ldr, int32_t r_is_y0,
                                                           float* const* y, const int32_t* out_rows, const int64_t* ldy, int32_t row_off,
                                                           int32_t offset_on_device)
{
    if (!codes || !scales || !scale_rows || !scale_cols || !n || !x || !y || !out_rows || !ldy) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const ProjShape s = check_fused_proj(mode, n, k, rows_alloc, ldx, rows, r, ldr, r_is_y0, y, out_rows, ldy, row_off);
        int kind[3] = {0, 0, 0};
        for (int i = 0; i < s.n_mats; ++i) {
            if (!codes[i] || !scales[i]) throw InvalidConfig("a matrix of this mode is NULL");
            kind[i] = fp8_scale_kind(n[i], k, scale_rows[i], scale_cols[i]);
            if (kind[i] < 0)
                throw InvalidConfig("FP8 projection: a scale of shape [" + std::to_string(scale_rows[i]) + ", " + std::to_string(scale_cols[i]) +
                                    "] is neither [1, 1] (per tensor), [n, 1] (per channel) nor [ceil(n / 128), k / 128] (block)");
            const uint8_t* c = static_cast<const uint8_t*>(codes[i]);
            for (int64_t e = 0, end = (int64_t)n[i] * k; e < end; ++e)
                if ((c[e] & 0x7F) == 0x7F) throw InvalidConfig("FP8 projection: NaN code at element " + std::to_string(e));
        }
        use_device(device);
        std::vector<std::unique_ptr<DeviceBuf>> keep;
        Fp8ProjArgs a;
        a.mode = mode == 1 ? F8_QKV : (mode == 2 ? F8_SWIGLU : F8_PLAIN);
        for (int i = 0; i < s.n_mats; ++i) {
            keep.push_back(upload(codes[i], (size_t)n[i] * k, "H2D codes"));
            a.W[i].codes = static_cast<const uint8_t*>(keep.back()->p);
            keep.push_back(upload(scales[i], (size_t)scale_rows[i] * scale_cols[i] * 4, "H2D scales"));
            a.W[i].scale = static_cast<const float*>(keep.back()->p);
            a.W[i].n = n[i]; a.W[i].k = k; a.W[i].kind = kind[i];
        }
        const auto xd = upload(x, (size_t)rows_alloc * (size_t)ldx * 4, "H2D x");
        const auto gd = upload(gamma, (size_t)k * 4, "H2D gamma");
        const auto bd = upload(bias, (size_t)s.n_tot * 4, "H2D bias");
        const auto rd = upload(r, (size_t)std::max(rows, 1) * (size_t)ldr * 4, "H2D r");
        const auto od = upload(&row_off, sizeof(int), "H2D row_off");
        const ProjOutputs out(s, y, out_rows, ldy);
        a.X = static_cast<const float*>(xd->p); a.ldx = ldx; a.rows = rows;
        a.gamma = gamma ? static_cast<const float*>(gd->p) : nullptr; a.eps = eps;
        a.bias = bias ? static_cast<const float*>(bd->p) : nullptr;
        if (r_is_y0) {
            a.R = out.dev(0); a.ldr = ldy[0];
        } else if (r) {
            a.R = static_cast<const float*>(rd->p); a.ldr = ldr;
        }
        for (int i = 0; i < s.n_outs; ++i) {
            a.Y[i] = out.dev(i); a.ldy[i] = ldy[i];
        }
        a.row_off = row_off;
        if (offset_on_device) {
            a.row_off_ptr = static_cast<const int*>(od->p);
            a.row_off = decoy_offset(row_off, mode == 1 ? std::min(out_rows[1], out_rows[2]) - rows : 0);
        }
        launcher_check(launch_fp8_proj(a, nullptr), "fp8 projection");
        hip_check(hipDeviceSynchronize(), "sync");
        out.fetch(y);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_fused_proj_ggml(int32_t device, int32_t mode, const void* const* blocks, const int32_t* ggml_types,
                                                            const int32_t* n, int32_t k, const float* x, int32_t rows_alloc, int64_t ldx,
                                                            int32_t rows, const float* gamma, float eps, const float* bias, int32_t bias_floats,
                                                            const int32_t* bias_off, const float* r, int64_t ldr, int32_t r_is_y0,
                                                            float* const* y, const int32_t* out_rows, const int64_t* ldy, int32_t row_off,
                                                            int32_t offset_on_device, int32_t head_dim, const float* cos_t, const float* sin_t,
                                                            int32_t positions, int32_t q8k, float* xn_out, int8_t* xq_out, float* xd_out)
{
    if (!blocks || !ggml_types || !n || !x || !y || !out_rows || !ldy) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const ProjShape s = check_fused_proj(mode, n, k, rows_alloc, ldx, rows, r, ldr, r_is_y0, y, out_rows, ldy, row_off);
        for (int i = 0; i < s.n_mats; ++i) {
            if (!blocks[i]) throw InvalidConfig("a matrix of this mode is NULL");
            check_qmat_type(ggml_types[i], k);
        }
        if (bias) {
            if (!bias_off) throw InvalidConfig("a bias needs bias_off[3]");
            for (int i = 0; i < (mode == 2 ? 1 : s.n_mats); ++i)
                if (bias_off[i] < 0 || (int64_t)bias_off[i] + n[i] > bias_floats) throw InvalidConfig("bias_off + the segment's columns exceed bias_floats");
        }
        if (mode == 1) {  // Q and K are rotated in the epilogue: whole heads, and a table row for every position
            if (head_dim < 2 || (head_dim & 1) || n[0] % head_dim || n[1] % head_dim || !cos_t || !sin_t)
                throw InvalidConfig("Q | K | V needs an even head_dim dividing the Q and K rows, and cos / sin tables");
            if (positions < 1 || (int64_t)row_off + rows > positions)
                throw InvalidConfig("positions " + std::to_string(row_off) + " .. +" + std::to_string(rows) + " are past the table's " +
                                    std::to_string(positions) + " rows");
        }
        use_device(device);
        std::vector<std::unique_ptr<DeviceBuf>> keep;
        QFusedArgs a;
        a.mode = mode == 1 ? QF_QKV : (mode == 2 ? QF_SWIGLU : QF_PLAIN);
        for (int i = 0; i < s.n_mats; ++i) a.W[i] = upload_qmat(ggml_types[i], blocks[i], n[i], k, keep);
        if (mode == 1) {  // (LlmModel::step_qkv: a job is a pair of columns)
            a.seg_jobs[0] = n[0] / 2; a.seg_jobs[1] = n[1] / 2; a.seg_jobs[2] = (n[2] + 1) / 2;
            a.jobs = a.seg_jobs[0] + a.seg_jobs[1] + a.seg_jobs[2];
        } else if (mode == 2) {
            a.jobs = n[0];
        } else {
            a.seg_jobs[0] = a.jobs = (n[0] + 1) / 2;
        }
        const int nb = k / 256;
        const auto xd = upload(x, (size_t)rows_alloc * (size_t)ldx * 4, "H2D x");
        const auto gd = upload(gamma, (size_t)k * 4, "H2D gamma");
        const auto bd = upload(bias, bias ? (size_t)bias_floats * 4 : 0, "H2D bias");
        const auto rd = upload(r, (size_t)std::max(rows, 1) * (size_t)ldr * 4, "H2D r");
        const auto od = upload(&row_off, sizeof(int), "H2D row_off");
        const size_t tb = mode == 1 ? (size_t)positions * (size_t)(head_dim / 2) * 4 : 0;
        const auto cd = upload(mode == 1 ? cos_t : nullptr, tb, "H2D cos"), sd = upload(mode == 1 ? sin_t : nullptr, tb, "H2D sin");
        const size_t rk = (size_t)std::max(rows, 1) * (size_t)k;
        GuardedBuf xn(rk * 4), xq(rk), xs((size_t)std::max(rows, 1) * (size_t)std::max(nb, 1) * 4);
        const ProjOutputs out(s, y, out_rows, ldy);
        a.k = k; a.rows = rows;
        const float* G = gamma ? static_cast<const float*>(gd->p) : nullptr;
        if (!q8k) {  // (LlmModel::quant_source)
            a.X = static_cast<const float*>(xd->p); a.ldx = ldx; a.gamma = G; a.eps = eps;
        } else {
            launcher_check(launch_qprep(static_cast<const float*>(xd->p), ldx, rows, k, G, eps, G ? xn.as<float>() : nullptr, xq.as<int8_t>(),
                                        xs.as<float>(), nullptr), "qprep");
            a.X = G ? xn.as<float>() : static_cast<const float*>(xd->p); a.ldx = G ? k : ldx; a.Xq = xq.as<int8_t>(); a.Xd = xs.as<float>();
        }
        if (bias) {
            a.bias = static_cast<const float*>(bd->p);
            for (int i = 0; i < 3; ++i) a.bias_off[i] = i < s.n_mats ? bias_off[i] : 0;
        }
        if (r_is_y0) {
            a.R = out.dev(0); a.ldr = ldy[0];
        } else if (r) {
            a.R = static_cast<const float*>(rd->p); a.ldr = ldr;
        }
        for (int i = 0; i < s.n_outs; ++i) {
            a.Y[i] = out.dev(i); a.ldy[i] = ldy[i];
        }
        a.row_off = row_off;
        if (offset_on_device) {
            a.row_off_ptr = static_cast<const int*>(od->p);
            a.row_off = decoy_offset(row_off, mode == 1 ? std::min(std::min(out_rows[1], out_rows[2]), positions) - rows : 0);
        }
        if (mode == 1) {
            a.head_dim = head_dim; a.cos_t = static_cast<const float*>(cd->p); a.sin_t = static_cast<const float*>(sd->p);
        }
        launcher_check(launch_qfused(a, nullptr), "quantized projection");
        hip_check(hipDeviceSynchronize(), "sync");
        out.fetch(y);
        if (q8k) {
            xn.check("normalised rows"); xq.check("Q8_K codes"); xs.check("Q8_K scales");
            if (xn_out && G) hip_check(hipMemcpy(xn_out, xn.buf.p, rk * 4, hipMemcpyDeviceToHost), "D2H xn");
            if (xq_out) hip_check(hipMemcpy(xq_out, xq.buf.p, rk, hipMemcpyDeviceToHost), "D2H codes");
            if (xd_out) hip_check(hipMemcpy(xd_out, xs.buf.p, (size_t)rows * nb * 4, hipMemcpyDeviceToHost), "D2H scales");
        }
    });
}

// ---- the dense (f32 / bf16) decode-step projections, alone ---------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_llm_gemv(int32_t device, int32_t lanes, const float* x, int32_t x_rows, int64_t ldx, int32_t rows,
                                                     const float* gamma, const float* beta, float eps, int32_t layernorm, int32_t gelu_tanh,
                                                     const void* w, const void* w2, int32_t bf16, int32_t swiglu, const float* bias,
                                                     const float* r, int64_t ldr, int32_t r_is_y0, int32_t n_out, int32_t k, int32_t seg_q,
                                                     int32_t seg_kv, float* const* y, const int32_t* out_rows, int64_t ldy0, int64_t ldy12,
                                                     int32_t row_off, int32_t offset_on_device, float* norm_out, int32_t* route_out)
{
    if (!x || !w || !y || !out_rows || !route_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // every element a kernel may read or write lies inside the buffers uploaded below
        if (lanes != 0 && lanes != 1) throw InvalidConfig("lanes must be 0 (launch_llm_gemv) or 1 (launch_llm_gemv_lanes)");
        if (rows < 0 || rows > 8 || x_rows < std::max(rows, 1) || x_rows > 64) throw InvalidConfig("rows must be 0 .. 8 and x_rows max(rows, 1) .. 64");
        if (n_out < 1 || k < 8 || n_out > (1 << 17) || k > (1 << 16) || (int64_t)n_out * k > ((int64_t)1 << 26))
            throw InvalidConfig("n_out must be 1 .. 2^17, k 8 .. 2^16, n_out * k at most 2^26");
        if ((k & 7) || (ldx & 3)) throw InvalidConfig("launch_llm_gemv refuses these arguments: k a multiple of 8, ldx a multiple of 4");
        if (ldx < k || ldx > (1 << 18)) throw InvalidConfig("ldx must cover k (at most 2^18)");
        if (layernorm && (!gamma || !beta || r || r_is_y0 || swiglu || norm_out))
            throw InvalidConfig("launch_llm_gemv refuses these arguments: LayerNorm needs gamma and beta and takes no residual, SwiGLU or norm_out");
        if (gelu_tanh && (!layernorm || seg_q != 0)) throw InvalidConfig("launch_llm_gemv refuses these arguments: GELU-tanh comes after LayerNorm, without segments");
        if (r && r_is_y0) throw InvalidConfig("r_is_y0 takes the residual from y[0]: r must be NULL");
        const bool res = r || r_is_y0;
        if (swiglu && !w2) throw InvalidConfig("SwiGLU needs w2");
        if ((swiglu && (!gamma || res)) || (res && gamma))
            throw InvalidConfig("launch_llm_gemv refuses these arguments: SwiGLU comes after RMSNorm without a residual, a residual without a norm");
        if (norm_out && !(rows == 1 && seg_q == 0 && gamma && (k == 2048 || k == 4096 || k == 8192)))
            throw InvalidConfig("launch_llm_gemv refuses these arguments: norm_out needs one row, gamma, no segments and k 2048 / 4096 / 8192");
        if (seg_q < 0 || seg_kv < 0 || (seg_q == 0 && seg_kv != 0)) throw InvalidConfig("seg_q and seg_kv must not be negative; seg_kv needs seg_q");
        const bool seg = seg_q > 0;
        if (seg && (seg_kv < 1 || (int64_t)seg_q + 2 * (int64_t)seg_kv != n_out)) throw InvalidConfig("seg_q + 2 * seg_kv must be n_out");
        if (seg && r_is_y0) throw InvalidConfig("no in-place residual with segments: y[0] holds seg_q of the n_out columns");
        if (row_off < 0) throw InvalidConfig("row_off must not be negative");
        const int n_outs = seg ? 3 : 1;
        const int64_t cols[3] = {seg ? seg_q : n_out, seg_kv, seg_kv}, ldy[3] = {ldy0, ldy12, ldy12};
        for (int i = 0; i < n_outs; ++i) {
            if (!y[i]) throw InvalidConfig("an output of this call is NULL");
            if (ldy[i] < cols[i] || ldy[i] > (1 << 18) || out_rows[i] < 1 || out_rows[i] > 4096 || (int64_t)out_rows[i] * ldy[i] > ((int64_t)1 << 24))
                throw InvalidConfig("ldy must cover the output's columns (at most 2^18); out_rows 1 .. 4096; at most 2^24 elements");
            if ((int64_t)(i == 0 ? 0 : row_off) + rows > out_rows[i])
                throw InvalidConfig("rows " + std::to_string(i == 0 ? 0 : row_off) + " .. +" + std::to_string(rows) + " do not fit the " +
                                    std::to_string(out_rows[i]) + " rows of output " + std::to_string(i));
        }
        if (r && (ldr < n_out || ldr > (1 << 18))) throw InvalidConfig("ldr must cover n_out (at most 2^18)");
        use_device(device);
        const size_t wb = (size_t)n_out * (size_t)k * (bf16 ? 2 : 4);
        const auto xd = upload(x, (size_t)x_rows * (size_t)ldx * 4, "H2D x");
        const auto gd = upload(gamma, (size_t)k * 4, "H2D gamma"), bed = upload(beta, (size_t)k * 4, "H2D beta");
        const auto wd = upload(w, wb, "H2D w"), w2d = upload(w2, w2 ? wb : 0, "H2D w2");
        const auto bd = upload(bias, (size_t)n_out * 4, "H2D bias");
        const auto rd = upload(r, r ? (size_t)std::max(rows, 1) * (size_t)ldr * 4 : 0, "H2D r");
        const auto od = upload(&row_off, sizeof(int), "H2D row_off");
        std::vector<std::unique_ptr<GuardedBuf>> out;
        for (int i = 0; i < n_outs; ++i) {
            out.push_back(std::make_unique<GuardedBuf>((size_t)out_rows[i] * (size_t)ldy[i] * 4));
            hip_check(hipMemcpy(out.back()->buf.p, y[i], out.back()->bytes, hipMemcpyHostToDevice), "H2D y");
        }
        GuardedBuf nd((size_t)k * 4);
        if (norm_out) hip_check(hipMemcpy(nd.buf.p, norm_out, (size_t)k * 4, hipMemcpyHostToDevice), "H2D norm_out");
        LlmGemvArgs a;
        a.X = static_cast<const float*>(xd->p); a.ldx = ldx; a.rows = rows;
        a.gamma = gamma ? static_cast<const float*>(gd->p) : nullptr; a.beta = beta ? static_cast<const float*>(bed->p) : nullptr;
        a.eps = eps; a.layernorm = layernorm ? 1 : 0; a.gelu_tanh = gelu_tanh ? 1 : 0;
        a.W = wd->p; a.W2 = w2 ? w2d->p : nullptr; a.bf16 = bf16 ? 1 : 0; a.swiglu = swiglu ? 1 : 0;
        a.bias = bias ? static_cast<const float*>(bd->p) : nullptr;
        if (r_is_y0) {
            a.R = out[0]->as<float>(); a.ldr = ldy0;
        } else if (r) {
            a.R = static_cast<const float*>(rd->p); a.ldr = ldr;
        }
        a.n_out = n_out; a.k = k; a.seg_q = seg_q; a.seg_kv = seg_kv;
        a.Y0 = out[0]->as<float>(); a.ldy0 = ldy0;
        if (seg) {
            a.Y1 = out[1]->as<float>(); a.Y2 = out[2]->as<float>(); a.ldy12 = ldy12;
        }
        a.row_off = row_off;
        if (offset_on_device) {
            a.row_off_ptr = static_cast<const int*>(od->p);
            a.row_off = decoy_offset(row_off, seg ? std::min(out_rows[1], out_rows[2]) - rows : 0);
        }
        a.norm_out = norm_out ? nd.as<float>() : nullptr;
        int32_t route[16] = {0};
        const LlmGemvRoute g = llm_gemv_route(a);
        const int32_t gr[7] = {g.kernel, g.ch, g.wide, g.threads, g.loop, g.rows_per_batch, g.workgroups};
        if (lanes) {
            const LlmGemvLanesRoute l = llm_gemv_lanes_route(a);
            int streamed = -1;
            launcher_check(launch_llm_gemv_lanes(a, nullptr, &streamed), "llm gemv, lanes");
            const int32_t lr[7] = {l.taken, l.ch, l.ns, l.wide, l.cpw, l.workgroups, streamed};
            std::copy(lr, lr + 7, route);
            if (!l.taken) std::copy(gr, gr + 7, route + 8);  // the fallback's own route
        } else {
            launcher_check(launch_llm_gemv(a, nullptr), "llm gemv");
            std::copy(gr, gr + 7, route);
        }
        hip_check(hipDeviceSynchronize(), "sync");
        for (int i = 0; i < n_outs; ++i) {
            out[i]->check("llm gemv output");
            hip_check(hipMemcpy(y[i], out[i]->buf.p, (size_t)out_rows[i] * (size_t)ldy[i] * 4, hipMemcpyDeviceToHost), "D2H y");
        }
        nd.check("norm_out");
        if (norm_out) hip_check(hipMemcpy(norm_out, nd.buf.p, (size_t)k * 4, hipMemcpyDeviceToHost), "D2H norm_out");
        std::copy(route, route + 16, route_out);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_llm_qkv_rope(int32_t device, const float* x, const uint32_t* embed_ids, const void* table, int32_t vocab,
                                                         const float* gamma, float eps, const void* w, int32_t bf16, const float* bias, int32_t k,
                                                         int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const float* cos_t,
                                                         const float* sin_t, int32_t positions, int32_t pos, int32_t offset_on_device, float* q,
                                                         float* k_cache, float* v_cache, int32_t cache_rows, float* x_raw_out, int32_t* route)
{
    if (!w || !cos_t || !sin_t || !q || !k_cache || !v_cache || !route) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (!gamma) throw InvalidConfig("launch_llm_qkv_rope refuses these arguments: gamma is NULL (both kernels normalise the row)");
        if (k < 8 || (k & 7) || k > 8192 || head_dim < 2 || (head_dim & 1))
            throw InvalidConfig("launch_llm_qkv_rope refuses these arguments: k a multiple of 8 and at most 8192, head_dim even");
        if (head_dim > 1024 || n_heads < 1 || n_heads > 256 || n_kv_heads < 1 || n_kv_heads > n_heads)
            throw InvalidConfig("head_dim at most 1024, n_heads 1 .. 256, n_kv_heads 1 .. n_heads");
        const int64_t q_dim = (int64_t)n_heads * head_dim, kv_dim = (int64_t)n_kv_heads * head_dim, n_out = q_dim + 2 * kv_dim;
        if (n_out * k > ((int64_t)1 << 26)) throw InvalidConfig("(n_heads + 2 n_kv_heads) * head_dim * k at most 2^26");
        if (!x == !embed_ids) throw InvalidConfig("the input row is x or the embedding of *embed_ids: exactly one of them");
        if (embed_ids) {
            if (!table || vocab < 1 || vocab > (1 << 17) || (int64_t)vocab * k > ((int64_t)1 << 26))
                throw InvalidConfig("the embedding gather needs a table, vocab 1 .. 2^17 and vocab * k at most 2^26");
            if (k != 2048 && k != 4096 && k != 8192) throw InvalidConfig("launch_llm_qkv_rope refuses these arguments: the gather needs k 2048 / 4096 / 8192");
        } else if (table || x_raw_out) {
            throw InvalidConfig("table and x_raw_out belong to the embedding gather");
        }
        if (positions < 1 || positions > (1 << 20) || cache_rows < 1 || cache_rows > 4096 || (int64_t)cache_rows * kv_dim > ((int64_t)1 << 24))
            throw InvalidConfig("positions must be 1 .. 2^20, cache_rows 1 .. 4096, a cache at most 2^24 elements");
        if (pos < 0 || pos >= positions || pos >= cache_rows) throw InvalidConfig("pos is no row of the tables or of the caches");
        use_device(device);
        const int half = head_dim / 2;
        const size_t es = bf16 ? 2 : 4, tb = (size_t)positions * (size_t)half * 4, cb = (size_t)cache_rows * (size_t)kv_dim * 4;
        const auto xd = upload(x, x ? (size_t)k * 4 : 0, "H2D x");
        const auto idd = upload(embed_ids, embed_ids ? 4 : 0, "H2D id");
        const auto td = upload(table, embed_ids ? (size_t)vocab * (size_t)k * es : 0, "H2D table");
        const auto gd = upload(gamma, (size_t)k * 4, "H2D gamma");
        const auto wd = upload(w, (size_t)n_out * (size_t)k * es, "H2D w");
        const auto bd = upload(bias, bias ? (size_t)n_out * 4 : 0, "H2D bias");
        const auto cd = upload(cos_t, tb, "H2D cos"), sd = upload(sin_t, tb, "H2D sin");
        const auto pd = upload(&pos, sizeof(int), "H2D pos");
        GuardedBuf qd((size_t)q_dim * 4), kd(cb), vd(cb), rd((size_t)k * 4);
        hip_check(hipMemcpy(qd.buf.p, q, (size_t)q_dim * 4, hipMemcpyHostToDevice), "H2D q");
        hip_check(hipMemcpy(kd.buf.p, k_cache, cb, hipMemcpyHostToDevice), "H2D k_cache");
        hip_check(hipMemcpy(vd.buf.p, v_cache, cb, hipMemcpyHostToDevice), "H2D v_cache");
        if (x_raw_out) hip_check(hipMemcpy(rd.buf.p, x_raw_out, (size_t)k * 4, hipMemcpyHostToDevice), "H2D x_raw_out");
        const float* G = static_cast<const float*>(gd->p);
        const uint32_t* ids = embed_ids ? static_cast<const uint32_t*>(idd->p) : nullptr;
        // (with the position on the device the by-value one is another row of the tables and the caches)
        const int by_value = offset_on_device ? decoy_offset(pos, std::min(positions, cache_rows) - 1) : pos;
        const LlmQkvRopeRoute rt = llm_qkv_rope_route(k, G, wd->p, n_heads, n_kv_heads, head_dim, ids);
        launcher_check(launch_llm_qkv_rope(x ? static_cast<const float*>(xd->p) : nullptr, G, eps, wd->p, bf16 ? 1 : 0,
                                           bias ? static_cast<const float*>(bd->p) : nullptr, k, n_heads, n_kv_heads, head_dim,
                                           static_cast<const float*>(cd->p), static_cast<const float*>(sd->p), qd.as<float>(), kd.as<float>(),
                                           vd.as<float>(), by_value, offset_on_device ? static_cast<const int*>(pd->p) : nullptr, nullptr, ids,
                                           embed_ids ? td->p : nullptr, embed_ids ? vocab : 0, x_raw_out ? rd.as<float>() : nullptr),
                       "llm qkv + rope");
        hip_check(hipDeviceSynchronize(), "sync");
        qd.check("q"); kd.check("k_cache"); vd.check("v_cache"); rd.check("x_raw_out");
        hip_check(hipMemcpy(q, qd.buf.p, (size_t)q_dim * 4, hipMemcpyDeviceToHost), "D2H q");
        hip_check(hipMemcpy(k_cache, kd.buf.p, cb, hipMemcpyDeviceToHost), "D2H k_cache");
        hip_check(hipMemcpy(v_cache, vd.buf.p, cb, hipMemcpyDeviceToHost), "D2H v_cache");
        if (x_raw_out) hip_check(hipMemcpy(x_raw_out, rd.buf.p, (size_t)k * 4, hipMemcpyDeviceToHost), "D2H x_raw_out");
        route[0] = rt.kernel; route[1] = rt.ch; route[2] = rt.workgroups;
    });
}

// ---- the Whisper decoder's row projections and the front-end kernels, alone ------------------------------------------------------

namespace {

// A device copy of `floats` host floats that starts `shift` floats (0 or 1) past a 16-byte boundary.
struct ShiftedBuf {
    DeviceBuf buf;
    int shift;
    ShiftedBuf(const float* src, size_t floats, int shift_, const char* what) : buf((floats + 1) * 4), shift(shift_)
    {
        if (src && floats) hip_check(hipMemcpy(static_cast<float*>(buf.p) + shift, src, floats * 4, hipMemcpyHostToDevice), what);
    }
    const float* p() const { return static_cast<const float*>(buf.p) + shift; }
};

// A whole host array on the device with a guard band behind it, and back.
struct RoundTrip {
    GuardedBuf d;
    float* host;
    RoundTrip(float* h, size_t floats) : d(floats * 4), host(h)
    {
        if (h && floats) hip_check(hipMemcpy(d.buf.p, h, floats * 4, hipMemcpyHostToDevice), "H2D output");
    }
    float* p() const { return d.as<float>(); }
    void fetch(const char* what, size_t floats) const
    {
        d.check(what);
        if (host && floats) hip_check(hipMemcpy(host, d.buf.p, floats * 4, hipMemcpyDeviceToHost), "D2H output");
    }
};

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_gemv_rows(int32_t device, const float* x, int32_t x_rows, int64_t ldx, int32_t rows, const float* gamma,
                                                      const float* beta, float eps, const float* w, const float* bias, const float* r,
                                                      int64_t ldr, int32_t r_is_y0, int32_t n_out, int32_t k, int32_t seg, float* const* y,
                                                      const int32_t* out_rows, int64_t ldy0, int64_t ldy12, int32_t row_off,
                                                      int32_t offset_on_device, int32_t epi, const uint32_t* embed_id, const float* embed_word,
                                                      int32_t embed_vocab, const float* embed_pos_table, int32_t embed_max_pos,
                                                      int32_t embed_pos, int32_t embed_pos_on_device, float embed_scale, float* x_raw_out,
                                                      float* x_norm_out, int32_t misalign, int32_t* route_out)
{
    if (!w || !y || !out_rows || !route_out || (!x && !embed_id)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // every element a kernel may read or write lies inside the buffers uploaded below
        if (rows < -1 || rows > 16 || x_rows < std::max(rows, 1) || x_rows > 64) throw InvalidConfig("rows must be -1 .. 16 and x_rows max(rows, 1) .. 64");
        if (n_out < -1 || k < 1 || n_out > (1 << 17) || k > (1 << 16) || (int64_t)std::max(n_out, 1) * k > ((int64_t)1 << 26))
            throw InvalidConfig("n_out must be -1 .. 2^17, k 1 .. 2^16, n_out * k at most 2^26");
        if (ldx < k || ldx > (1 << 18)) throw InvalidConfig("ldx must cover k (at most 2^18)");
        if (epi < 0 || epi > (int)EPI_BIAS_MUL_SILU) throw InvalidConfig("epi is no epilogue");
        if (misalign < 0 || misalign > 15) throw InvalidConfig("misalign is a mask of X (1), W (2), gamma (4), beta (8)");
        if (r && r_is_y0) throw InvalidConfig("r_is_y0 takes the residual from y[0]: r must be NULL");
        if (seg < 0 || row_off < 0) throw InvalidConfig("seg and row_off must not be negative");
        if (seg > 0 && r_is_y0) throw InvalidConfig("no in-place residual with segments: y[0] holds seg of the n_out columns");
        const int nn = std::max(n_out, 1), n_outs = seg > 0 ? 3 : 1;
        const int64_t cols[3] = {seg > 0 ? seg : nn, seg, seg}, ldy[3] = {ldy0, ldy12, ldy12};
        for (int i = 0; i < n_outs; ++i) {
            if (!y[i]) throw InvalidConfig("an output of this call is NULL");
            if (ldy[i] < cols[i] || ldy[i] > (1 << 18) || out_rows[i] < 1 || out_rows[i] > 4096 || (int64_t)out_rows[i] * ldy[i] > ((int64_t)1 << 24))
                throw InvalidConfig("ldy must cover the output's columns (at most 2^18); out_rows 1 .. 4096; at most 2^24 elements");
            if ((int64_t)(i == 0 ? 0 : row_off) + std::max(rows, 0) > out_rows[i])
                throw InvalidConfig("rows " + std::to_string(i == 0 ? 0 : row_off) + " .. +" + std::to_string(rows) + " do not fit the " +
                                    std::to_string(out_rows[i]) + " rows of output " + std::to_string(i));
        }
        if (r && (ldr < nn || ldr > (1 << 18))) throw InvalidConfig("ldr must cover n_out (at most 2^18)");
        if (embed_id) {  // the word row id * k and the position row p * k are read only below vocab / max_pos: the tables hold that many rows
            if (embed_vocab < 0 || embed_vocab > (1 << 17) || (int64_t)embed_vocab * k > ((int64_t)1 << 26) || embed_max_pos < 0 ||
                embed_max_pos > (1 << 16) || embed_pos < 0)
                throw InvalidConfig("embed: vocab 0 .. 2^17 (vocab * k at most 2^26), max_pos 0 .. 2^16, pos not negative");
        } else if (embed_word || embed_pos_table || embed_pos_on_device) {
            throw InvalidConfig("embed_word, embed_pos_table and embed_pos_on_device belong to embed_id");
        }
        // The launcher's own refusals, asked of its rule before any GPU work: the rule looks at the pointers only for NULL and for
        // their alignment, which the uploads below reproduce.
        const auto fake = [](bool given, int shift) { return given ? reinterpret_cast<float*>((uintptr_t)4096 + 4 * (uintptr_t)shift) : nullptr; };
        const int sx = misalign & 1, sw = (misalign >> 1) & 1, sg = (misalign >> 2) & 1, sb = (misalign >> 3) & 1;
        GemvArgs a;
        a.X = fake(x != nullptr, sx); a.ldx = ldx; a.rows = rows; a.gamma = fake(gamma != nullptr, sg); a.beta = fake(beta != nullptr, sb);
        a.eps = eps; a.W = fake(true, sw); a.bias = fake(bias != nullptr, 0); a.R = fake(r || r_is_y0, 0); a.ldr = r_is_y0 ? ldy0 : ldr;
        a.n_out = n_out; a.k = k; a.seg = seg; a.Y0 = fake(true, 0); a.ldy0 = ldy0;
        if (seg > 0) {
            a.Y1 = fake(true, 0); a.Y2 = fake(true, 0); a.ldy12 = ldy12;
        }
        a.epi = (GemmEpilogue)epi;
        a.embed_ids = embed_id ? reinterpret_cast<const uint32_t*>(fake(true, 0)) : nullptr;
        a.embed_word = fake(embed_word != nullptr, 0); a.embed_pos_table = fake(embed_pos_table != nullptr, 0);
        a.embed_vocab = embed_vocab; a.embed_max_pos = embed_max_pos; a.embed_scale = embed_scale;
        a.x_raw_out = fake(x_raw_out != nullptr, 0); a.x_norm_out = fake(x_norm_out != nullptr, 0);
        const GemvRowsRoute route = gemv_rows_route(a);
        if (route == GEMV_ROWS_REFUSED) throw InvalidConfig("launch_gemv_rows refuses these arguments");
        use_device(device);
        const ShiftedBuf xd(x, x ? (size_t)x_rows * (size_t)ldx : 0, sx, "H2D x"), wd(w, (size_t)nn * (size_t)k, sw, "H2D w");
        const ShiftedBuf gd(gamma, (size_t)k, sg, "H2D gamma"), bed(beta, (size_t)k, sb, "H2D beta");
        const auto bd = upload(bias, (size_t)nn * 4, "H2D bias");
        const auto rd = upload(r, r ? (size_t)std::max(rows, 1) * (size_t)ldr * 4 : 0, "H2D r");
        const auto od = upload(&row_off, sizeof(int), "H2D row_off"), pd = upload(&embed_pos, sizeof(int), "H2D embed_pos");
        const auto idd = upload(embed_id, embed_id ? 4 : 0, "H2D embed_id");
        const auto wordd = upload(embed_word, embed_id ? (size_t)embed_vocab * (size_t)k * 4 : 0, "H2D embed_word");
        const auto posd = upload(embed_pos_table, embed_id ? (size_t)embed_max_pos * (size_t)k * 4 : 0, "H2D embed_pos_table");
        std::vector<std::unique_ptr<RoundTrip>> out;
        for (int i = 0; i < n_outs; ++i) out.push_back(std::make_unique<RoundTrip>(y[i], (size_t)out_rows[i] * (size_t)ldy[i]));
        const RoundTrip raw(x_raw_out, x_raw_out ? (size_t)k : 0), norm(x_norm_out, x_norm_out ? (size_t)k : 0);
        a.X = x ? xd.p() : nullptr; a.gamma = gamma ? gd.p() : nullptr; a.beta = beta ? bed.p() : nullptr; a.W = wd.p();
        a.bias = bias ? static_cast<const float*>(bd->p) : nullptr;
        a.R = r_is_y0 ? out[0]->p() : (r ? static_cast<const float*>(rd->p) : nullptr);
        a.Y0 = out[0]->p();
        if (seg > 0) {
            a.Y1 = out[1]->p(); a.Y2 = out[2]->p();
        }
        a.row_off = row_off;
        if (offset_on_device) {  // (the by-value copy is then another row inside both caches)
            a.row_off_ptr = static_cast<const int*>(od->p);
            a.row_off = decoy_offset(row_off, seg > 0 ? std::min(out_rows[1], out_rows[2]) - std::max(rows, 0) : 0);
        }
        if (embed_id) {
            a.embed_ids = static_cast<const uint32_t*>(idd->p);
            a.embed_word = embed_word ? static_cast<const float*>(wordd->p) : nullptr;
            a.embed_pos_table = embed_pos_table ? static_cast<const float*>(posd->p) : nullptr;
            a.embed_pos = embed_pos;
            if (embed_pos_on_device) {
                a.embed_pos_ptr = static_cast<const int*>(pd->p);
                a.embed_pos = decoy_offset(embed_pos, embed_max_pos - 1);
            }
        }
        a.x_raw_out = x_raw_out ? raw.p() : nullptr; a.x_norm_out = x_norm_out ? norm.p() : nullptr;
        expect(gemv_rows_route(a) == route, "the route changed between the check and the launch");
        launcher_check(launch_gemv_rows(a, nullptr), "gemv rows");
        hip_check(hipDeviceSynchronize(), "sync");
        for (int i = 0; i < n_outs; ++i) out[i]->fetch("gemv rows output", (size_t)out_rows[i] * (size_t)ldy[i]);
        raw.fetch("x_raw_out", x_raw_out ? (size_t)k : 0);
        norm.fetch("x_norm_out", x_norm_out ? (size_t)k : 0);
        *route_out = (int32_t)route;
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_gemv_rows_route(int32_t rows, int32_t n_out, int32_t k, int64_t ldx, int32_t seg, int32_t epi,
                                                         int32_t has_gamma, int32_t has_beta, int32_t has_r, int32_t embed, int32_t x_raw_out,
                                                         int32_t x_norm_out, int32_t misalign, int32_t* route_out)
{
    if (!route_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const auto fake = [](bool given, int shift) { return given ? reinterpret_cast<float*>((uintptr_t)4096 + 4 * (uintptr_t)shift) : nullptr; };
        GemvArgs a;
        a.X = fake(true, misalign & 1); a.ldx = ldx; a.rows = rows; a.gamma = fake(has_gamma != 0, (misalign >> 2) & 1);
        a.beta = fake(has_beta != 0, (misalign >> 3) & 1); a.W = fake(true, (misalign >> 1) & 1); a.R = fake(has_r != 0, 0);
        a.n_out = n_out; a.k = k; a.seg = seg; a.Y0 = fake(true, 0); a.Y1 = fake(seg > 0, 0); a.Y2 = fake(seg > 0, 0);
        a.epi = (GemmEpilogue)epi;
        a.embed_ids = embed ? reinterpret_cast<const uint32_t*>(fake(true, 0)) : nullptr; a.embed_word = fake(embed != 0, 0);
        a.x_raw_out = fake(x_raw_out != 0, 0); a.x_norm_out = fake(x_norm_out != 0, 0);
        *route_out = (int32_t)gemv_rows_route(a);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_mel_frames(int32_t device, const float* audio, int64_t n_samples, const float* window, int32_t n_fft,
                                                       int32_t hop, int32_t n_frames, int32_t ld, float* frames)
{
    if (!audio || !window || !frames) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // (the kernel's clamps keep every sample index inside [0, n_samples) once there is a sample; window [n_fft]; frames [n_frames, ld])
        if (n_samples < 1 || n_samples > (1 << 24) || n_fft < 2 || n_fft > 4096 || hop < 1 || hop > 4096 || n_frames < 1 || n_frames > (1 << 16) ||
            ld < n_fft || ld > 8192 || (int64_t)n_frames * ld > ((int64_t)1 << 24))
            throw InvalidConfig("mel_frames: n_samples 1 .. 2^24, n_fft 2 .. 4096, hop 1 .. 4096, n_frames 1 .. 2^16, ld n_fft .. 8192");
        use_device(device);
        const auto ad = upload(audio, (size_t)n_samples * 4, "H2D audio"), wd = upload(window, (size_t)n_fft * 4, "H2D window");
        const size_t fl = (size_t)n_frames * (size_t)ld;
        const RoundTrip fd(frames, fl);
        launcher_check(launch_mel_frames(static_cast<const float*>(ad->p), n_samples, static_cast<const float*>(wd->p), n_fft, hop, n_frames, ld,
                                         fd.p(), nullptr), "mel_frames");
        hip_check(hipDeviceSynchronize(), "sync");
        fd.fetch("frames", fl);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_mel_power(int32_t device, const float* dft, int32_t ld_dft, int32_t im_off, int32_t n_bins,
                                                      int32_t ld_out, int32_t n_frames, float* power)
{
    if (!dft || !power) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_frames < 1 || n_frames > (1 << 16) || n_bins < 0 || n_bins > ld_out || ld_out < 1 || ld_out > 8192 || im_off < 0 ||
            (int64_t)im_off + n_bins > ld_dft || ld_dft > 8192)
            throw InvalidConfig("mel_power: n_frames 1 .. 2^16, n_bins 0 .. ld_out, im_off + n_bins within ld_dft, strides at most 8192");
        use_device(device);
        const auto dd = upload(dft, (size_t)n_frames * (size_t)ld_dft * 4, "H2D dft");
        const size_t pl = (size_t)n_frames * (size_t)ld_out;
        const RoundTrip pw(power, pl);
        launcher_check(launch_mel_power(static_cast<const float*>(dd->p), ld_dft, im_off, n_bins, ld_out, n_frames, pw.p(), nullptr), "mel_power");
        hip_check(hipDeviceSynchronize(), "sync");
        pw.fetch("power", pl);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_mel_log_normalize(int32_t device, float* mel, int32_t ld, int32_t n_mels, int32_t n_frames,
                                                              int32_t ld_out, float* out)
{
    if (!mel || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_frames < 1 || n_frames > (1 << 16) || n_mels < 1 || ld < n_mels || ld_out < n_mels || ld > 4096 || ld_out > 4096)
            throw InvalidConfig("mel_log_normalize: n_frames 1 .. 2^16, n_mels 1 .. ld and ld_out, strides at most 4096");
        use_device(device);
        const size_t ml = (size_t)n_frames * (size_t)ld, ol = (size_t)n_frames * (size_t)ld_out;
        const RoundTrip md(mel, ml), od(out, ol);
        GuardedBuf mx(4);
        hip_check(hipMemset(mx.buf.p, 0xFF, 4), "poison max");  // (the launcher zeroes it itself)
        launcher_check(launch_mel_log_normalize(md.p(), ld, n_mels, n_frames, mx.as<uint32_t>(), ld_out, od.p(), nullptr), "mel_log_normalize");
        hip_check(hipDeviceSynchronize(), "sync");
        mx.check("max scratch");
        md.fetch("mel", ml);
        od.fetch("out", ol);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_im2col3(int32_t device, const float* x, int64_t ldx, int32_t t_in, int32_t channels, int32_t stride,
                                                    int32_t pad, int32_t t_out, int32_t ld_cols, float* cols)
{
    if (!x || !cols) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // (x [t_in, ldx]: the kernel tests every row it reads against [0, t_in); cols [t_out, ld_cols])
        if (t_in < 1 || t_in > (1 << 16) || channels < 1 || channels > 4096 || ldx < channels || ldx > 8192 || stride < 1 || stride > 16 || pad < 0 ||
            pad > 16 || t_out < 1 || t_out > (1 << 16) || ld_cols < 3 * channels || ld_cols > (1 << 14) || (int64_t)t_out * ld_cols > ((int64_t)1 << 24))
            throw InvalidConfig("im2col3: t_in, t_out 1 .. 2^16, channels 1 .. 4096 within ldx, stride 1 .. 16, pad 0 .. 16, ld_cols at least 3 channels");
        use_device(device);
        const auto xd = upload(x, (size_t)t_in * (size_t)ldx * 4, "H2D x");
        const size_t cl = (size_t)t_out * (size_t)ld_cols;
        const RoundTrip cd(cols, cl);
        launcher_check(launch_im2col3(static_cast<const float*>(xd->p), ldx, t_in, channels, stride, pad, t_out, ld_cols, cd.p(), nullptr), "im2col3");
        hip_check(hipDeviceSynchronize(), "sync");
        cd.fetch("cols", cl);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_add_rows(int32_t device, float* x, int32_t rows, int32_t hidden, int32_t period, const float* table,
                                                     int32_t table_rows, int32_t table_alloc_rows)
{
    if (!x || !table) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // (table [table_alloc_rows, hidden], of which the call may use the first table_rows)
        if (rows < 1 || rows > (1 << 16) || hidden < 1 || hidden > 8192 || period < 1 || table_rows < 0 || table_alloc_rows < std::max(table_rows, 1) ||
            table_alloc_rows > (1 << 16))
            throw InvalidConfig("add_rows: rows 1 .. 2^16, hidden 1 .. 8192, period at least 1, table_rows 0 .. table_alloc_rows (1 .. 2^16)");
        use_device(device);
        const auto td = upload(table, (size_t)table_alloc_rows * (size_t)hidden * 4, "H2D table");
        const size_t xl = (size_t)rows * (size_t)hidden;
        const RoundTrip xd(x, xl);
        launcher_check(launch_add_rows(xd.p(), rows, hidden, period, static_cast<const float*>(td->p), table_rows, nullptr), "add_rows");
        hip_check(hipDeviceSynchronize(), "sync");
        xd.fetch("x", xl);
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_decoder_embed(int32_t device, const uint32_t* ids, int32_t n, int32_t hidden, int32_t vocab,
                                                          const float* word, const float* pos, int32_t max_pos, int32_t offset,
                                                          int32_t offset_on_device, int32_t scale_embeddings, int32_t lanes, float* out)
{
    if (!ids || !word || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        // (word [vocab, hidden], pos [max_pos, hidden] or NULL: the kernel reads row id only below vocab, row p only below max_pos)
        if (n < 1 || n > 64 || hidden < 1 || hidden > 8192 || vocab < 1 || vocab > (1 << 17) || (int64_t)vocab * hidden > ((int64_t)1 << 26) ||
            max_pos < 0 || max_pos > (1 << 16) || offset < 0 || (pos && max_pos < 1))
            throw InvalidConfig("decoder_embed: n 1 .. 64, hidden 1 .. 8192, vocab 1 .. 2^17, max_pos 0 .. 2^16, offset not negative");
        use_device(device);
        const auto idd = upload(ids, (size_t)n * 4, "H2D ids");
        const auto wd = upload(word, (size_t)vocab * (size_t)hidden * 4, "H2D word"), pd = upload(pos, pos ? (size_t)max_pos * (size_t)hidden * 4 : 0, "H2D pos");
        const auto od = upload(&offset, sizeof(int), "H2D offset");
        const size_t ol = (size_t)n * (size_t)hidden;
        const RoundTrip out_d(out, ol);
        // (with the position on the device the by-value one is another row: the kernel stays inside the table for any of them)
        launcher_check(launch_decoder_embed(static_cast<const uint32_t*>(idd->p), n, hidden, vocab, static_cast<const float*>(wd->p),
                                            pos ? static_cast<const float*>(pd->p) : nullptr, max_pos,
                                            offset_on_device ? decoy_offset(offset, max_pos - 1) : offset,
                                            offset_on_device ? static_cast<const int*>(od->p) : nullptr, scale_embeddings ? 1 : 0, out_d.p(), nullptr,
                                            lanes ? 1 : 0), "decoder_embed");
        hip_check(hipDeviceSynchronize(), "sync");
        out_d.fetch("out", ol);
    });
}

// ---- wide lanes: the rotate-and-scatter launchers and the pick alone ------------------------------------------------------------

static_assert(sizeof(KjarniHipWideState) == sizeof(LlmWideState) && KJARNI_HIP_WIDE_LANES == kMaxWideLanes &&
                  KJARNI_HIP_LANE_STOPS == kMaxLaneStops, "the header's wide state is the kernels'");

KJARNI_EXPORT size_t kjarni_hip_wide_state_size(void) { return sizeof(LlmWideState); }

// ONE call of launch_lane_rope_scatter (gamma_q / gamma_k NULL) or launch_lane_qk_norm_rope_scatter (both given) over the
// 64-lane state layout on host arrays: qkv [lanes, ld] and k_cache / v_cache [lanes, lane_stride] are read, run and written back
// whole, each with a guard band behind it, so a caller can check what the call left untouched.  pos / live [lanes]; cos_t /
// sin_t [table_rows, head_dim / 2].
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_wide_rope_scatter(int32_t device, float* qkv, int64_t ld, int32_t lanes, int32_t n_heads,
                                                              int32_t n_kv_heads, int32_t head_dim, const float* gamma_q, const float* gamma_k,
                                                              float eps, const float* cos_t, const float* sin_t, int32_t table_rows,
                                                              float* k_cache, float* v_cache, int64_t lane_stride, int32_t capacity,
                                                              const int32_t* pos, const int32_t* live, int32_t rotate)
{
    if (!qkv || !cos_t || !sin_t || !k_cache || !v_cache || !pos || !live) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (!gamma_q != !gamma_k) throw InvalidConfig("gamma_q and gamma_k go together (both: the Qwen3 form, neither: the plain form)");
        if (gamma_q && !rotate) throw InvalidConfig("the Qwen3 form always rotates: rotate must be 1 with gamma_q / gamma_k");
        if (lanes < 1 || lanes > kMaxWideLanes) throw InvalidConfig("lanes must be 1..64");
        if (head_dim < 2 || head_dim > 128 || (head_dim & 1) || n_heads < 1 || n_heads > 256 || n_kv_heads < 1 || n_kv_heads > n_heads)
            throw InvalidConfig("invalid head geometry (head_dim even, 2..128; n_heads 1..256; n_kv_heads 1..n_heads)");
        const int64_t kv = (int64_t)n_kv_heads * head_dim, width = (int64_t)n_heads * head_dim + 2 * kv;
        if (ld < width || ld > ((int64_t)1 << 20)) throw InvalidConfig("ld does not cover Q | K | V (or exceeds 2^20)");
        if (capacity < 1 || capacity > (1 << 16) || lane_stride < (int64_t)capacity * kv || lane_stride > ((int64_t)1 << 24))
            throw InvalidConfig("capacity 1..2^16 rows, lane_stride at least capacity * kv floats and at most 2^24");
        if (table_rows < 1 || table_rows > (1 << 20)) throw InvalidConfig("table_rows must be 1..2^20");
        for (int32_t l = 0; l < lanes; ++l) {
            if (pos[l] < 0) throw InvalidConfig("pos[" + std::to_string(l) + "] is negative");
            if (live[l] && pos[l] < capacity && pos[l] >= table_rows)
                throw InvalidConfig("pos[" + std::to_string(l) + "] = " + std::to_string(pos[l]) + " is outside the RoPE tables");
        }
        use_device(device);
        const size_t qb = (size_t)lanes * (size_t)ld * 4, cb = (size_t)lanes * (size_t)lane_stride * 4, tb = (size_t)table_rows * (head_dim / 2) * 4;
        LlmWideState st = {};
        for (int32_t l = 0; l < lanes; ++l) {
            st.pos[l] = pos[l];
            st.live[l] = live[l] ? 1 : 0;
        }
        const auto sd = upload(&st, sizeof(st), "H2D state");
        const auto cd = upload(cos_t, tb, "H2D cos"), snd = upload(sin_t, tb, "H2D sin");
        const auto gq = upload(gamma_q, gamma_q ? (size_t)head_dim * 4 : 0, "H2D gamma_q"), gk = upload(gamma_k, gamma_k ? (size_t)head_dim * 4 : 0, "H2D gamma_k");
        GuardedBuf qd(qb), kd(cb), vd(cb);
        hip_check(hipMemcpy(qd.buf.p, qkv, qb, hipMemcpyHostToDevice), "H2D qkv");
        hip_check(hipMemcpy(kd.buf.p, k_cache, cb, hipMemcpyHostToDevice), "H2D k_cache");
        hip_check(hipMemcpy(vd.buf.p, v_cache, cb, hipMemcpyHostToDevice), "H2D v_cache");
        const LaneStateRef ds(static_cast<LlmWideState*>(sd->p));
        if (gamma_q)
            launcher_check(launch_lane_qk_norm_rope_scatter(qd.as<float>(), ld, lanes, n_heads, n_kv_heads, head_dim, static_cast<const float*>(gq->p),
                                                            static_cast<const float*>(gk->p), eps, static_cast<const float*>(cd->p),
                                                            static_cast<const float*>(snd->p), kd.as<float>(), vd.as<float>(), lane_stride, capacity,
                                                            ds, nullptr), "wide head norm + rotate + scatter");
        else
            launcher_check(launch_lane_rope_scatter(qd.as<float>(), ld, lanes, n_heads, n_kv_heads, head_dim, static_cast<const float*>(cd->p),
                                                    static_cast<const float*>(snd->p), kd.as<float>(), vd.as<float>(), lane_stride, capacity, ds,
                                                    rotate ? 1 : 0, nullptr), "wide rotate + scatter");
        hip_check(hipDeviceSynchronize(), "sync");
        qd.check("qkv"); kd.check("k_cache"); vd.check("v_cache");
        hip_check(hipMemcpy(qkv, qd.buf.p, qb, hipMemcpyDeviceToHost), "D2H qkv");
        hip_check(hipMemcpy(k_cache, kd.buf.p, cb, hipMemcpyDeviceToHost), "D2H k_cache");
        hip_check(hipMemcpy(v_cache, vd.buf.p, cb, hipMemcpyDeviceToHost), "D2H v_cache");
    });
}

// ONE call of launch_lane_pick over the 64-lane state layout on host arrays: logits [first_lane + lanes, ld], the state and
// history [64, hist_stride] read, picked over lanes [first_lane, first_lane + lanes) and written back whole; the scratch must
// come back zeroed.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_wide_pick(int32_t device, const float* logits, int64_t ld, int32_t vocab, int32_t lanes,
                                                      int32_t first_lane, KjarniHipWideState* state, int32_t* history, int32_t hist_stride,
                                                      int32_t capacity, int32_t advance)
{
    if (!logits || !state || !history) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (lanes < 1 || first_lane < 0 || first_lane > kMaxWideLanes - lanes) throw InvalidConfig("lanes [first_lane, first_lane + lanes) must lie in 0..64");
        if (vocab < 1 || ld < vocab || ld > (1 << 20)) throw InvalidConfig("vocab >= 1, vocab <= ld <= 2^20");
        if (hist_stride < 1 || hist_stride > (1 << 16) || capacity < 0) throw InvalidConfig("hist_stride 1..2^16, capacity >= 0");
        for (int l = first_lane; l < first_lane + lanes; ++l) {
            if (state->n_stop[l] < 0 || state->n_stop[l] > kMaxLaneStops) throw InvalidConfig("n_stop[" + std::to_string(l) + "] must be 0..16");
            if (state->live[l] && (state->count[l] < 0 || state->count[l] >= hist_stride))
                throw InvalidConfig("count[" + std::to_string(l) + "] is no entry of the lane's history");
        }
        use_device(device);
        const size_t lb = (size_t)(first_lane + lanes) * (size_t)ld * 4, hb = (size_t)kMaxWideLanes * (size_t)hist_stride * 4;
        const auto dl = upload(logits, lb, "H2D logits");
        GuardedBuf sd(sizeof(LlmWideState)), hd(hb), best(kMaxWideLanes * sizeof(unsigned long long));
        hip_check(hipMemcpy(sd.buf.p, state, sizeof(LlmWideState), hipMemcpyHostToDevice), "H2D state");
        hip_check(hipMemcpy(hd.buf.p, history, hb, hipMemcpyHostToDevice), "H2D history");
        hip_check(hipMemset(best.buf.p, 0, kMaxWideLanes * sizeof(unsigned long long)), "memset");
        launcher_check(launch_lane_pick(static_cast<const float*>(dl->p), ld, vocab, lanes, first_lane, best.as<unsigned long long>(),
                                        sd.as<LlmWideState>(), hd.as<int32_t>(), hist_stride, capacity, advance ? 1 : 0, nullptr), "wide pick");
        hip_check(hipDeviceSynchronize(), "sync");
        sd.check("wide state"); hd.check("wide history"); best.check("wide pick scratch");
        unsigned long long b[kMaxWideLanes];
        hip_check(hipMemcpy(b, best.buf.p, sizeof(b), hipMemcpyDeviceToHost), "D2H best");
        for (int i = 0; i < kMaxWideLanes; ++i) expect(b[i] == 0ull, "the wide pick left its accumulator non-zero");
        hip_check(hipMemcpy(state, sd.buf.p, sizeof(LlmWideState), hipMemcpyDeviceToHost), "D2H state");
        hip_check(hipMemcpy(history, hd.buf.p, hb, hipMemcpyDeviceToHost), "D2H history");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_qembed(int32_t device, const uint32_t* ids, int32_t n_ids, const void* blocks, int32_t ggml_type,
                                                   int32_t vocab, int32_t k, float* out)
{
    if (!ids || !blocks || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (n_ids < 1 || n_ids > 4096 || vocab < 1 || vocab > (1 << 20) || k < 1 || k > (1 << 20)) throw InvalidConfig("n_ids 1 .. 4096; vocab, k 1 .. 2^20");
        if (!ggml_matrix_type((uint32_t)ggml_type) || k % 256) throw InvalidConfig("a Q8_0 / Q4_K / Q6_K table with k % 256 == 0");
        use_device(device);
        std::vector<std::unique_ptr<DeviceBuf>> keep;
        const QMat table = upload_qmat(ggml_type, blocks, vocab, k, keep);
        const auto idd = upload(ids, (size_t)n_ids * 4, "H2D ids");
        const size_t ob = (size_t)n_ids * (size_t)k * 4;
        GuardedBuf od(ob);
        hip_check(hipMemcpy(od.buf.p, out, ob, hipMemcpyHostToDevice), "H2D out");
        launcher_check(launch_qembed(static_cast<const uint32_t*>(idd->p), n_ids, table, od.as<float>(), nullptr), "qembed");
        hip_check(hipDeviceSynchronize(), "sync");
        od.check("embedding rows");
        hip_check(hipMemcpy(out, od.buf.p, ob, hipMemcpyDeviceToHost), "D2H out");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_q8k_quantize(int32_t device, const float* x, int32_t rows, int64_t ldx, int32_t k, int8_t* codes_out,
                                                         float* scales_out, float* deq_out)
{
    if (!x || !codes_out || !scales_out || !deq_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > 64 || k < 1 || k > (1 << 20) || k % 256 || ldx < k || (ldx & 3) || ldx > (1 << 21))
            throw InvalidConfig("rows 1 .. 64; k a multiple of 256; ldx a multiple of 4 covering k");
        use_device(device);
        const auto xd = upload(x, (size_t)rows * (size_t)ldx * 4, "H2D x");
        const size_t rk = (size_t)rows * (size_t)k, sb = (size_t)rows * (k / 256) * 4;
        GuardedBuf cd(rk), sd(sb), dd(rk * 4);
        launcher_check(launch_q8k_quantize(static_cast<const float*>(xd->p), ldx, rows, k, cd.as<int8_t>(), sd.as<float>(), dd.as<float>(), nullptr),
                       "q8k quantize");
        hip_check(hipDeviceSynchronize(), "sync");
        cd.check("Q8_K codes"); sd.check("Q8_K scales"); dd.check("Q8_K deq");
        hip_check(hipMemcpy(codes_out, cd.buf.p, rk, hipMemcpyDeviceToHost), "D2H codes");
        hip_check(hipMemcpy(scales_out, sd.buf.p, sb, hipMemcpyDeviceToHost), "D2H scales");
        hip_check(hipMemcpy(deq_out, dd.buf.p, rk * 4, hipMemcpyDeviceToHost), "D2H deq");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_score_head(int32_t device, const float* hidden, int64_t m, int32_t k, const void* W, int32_t bf16,
                                                       int32_t vocab, const uint32_t* targets, int32_t slab_tiles, int32_t fused,
                                                       float* logprob_out, uint32_t* top_out, float* top_logprob_out, float* lse_out)
{
    if (!hidden || !W || !targets) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || m > (1 << 20) || k <= 0 || vocab <= 0 || slab_tiles < 0 || (bf16 != 0 && bf16 != 1))
            throw InvalidConfig("invalid score head dimensions");
        if (fused ? k % 32 != 0 : k % 8 != 0) throw InvalidConfig(fused ? "the fused score head needs k % 32 == 0" : "the rows route needs k % 8 == 0");
        for (int64_t r = 0; r < m; ++r)
            if (targets[r] >= (uint32_t)vocab) throw InvalidConfig("targets[" + std::to_string(r) + "] is not below vocab");
        use_device(device);
        if (m == 0) return;
        const size_t xb = (size_t)m * k * 4, wb = (size_t)vocab * k * (bf16 ? 2 : 4), ob = (size_t)m * 4;
        DeviceBuf xd(xb), wd(wb), td(ob), lp(ob), tp(ob), tl(ob), ls(ob);
        hip_check(hipMemcpy(xd.p, hidden, xb, hipMemcpyHostToDevice), "H2D hidden");
        hip_check(hipMemcpy(wd.p, W, wb, hipMemcpyHostToDevice), "H2D W");
        hip_check(hipMemcpy(td.p, targets, ob, hipMemcpyHostToDevice), "H2D targets");
        const float* X = static_cast<const float*>(xd.p);
        const uint32_t* T = static_cast<const uint32_t*>(td.p);
        float *LP = static_cast<float*>(lp.p), *TL = static_cast<float*>(tl.p), *LS = static_cast<float*>(ls.p);
        uint32_t* TP = static_cast<uint32_t*>(tp.p);
        if (fused) {
            DeviceBuf scratch(score_head_scratch_bytes((int)m, vocab, slab_tiles));
            hip_check(launch_score_head(X, k, (int)m, wd.p, bf16, vocab, k, T, slab_tiles, scratch.p, LP, TP, TL, LS, nullptr), "score head");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        } else {
            DeviceBuf logits((size_t)8 * vocab * 4);
            for (int64_t r = 0; r < m; r += 8) {
                LlmGemvArgs a;
                a.X = X + r * k; a.ldx = k; a.rows = (int)std::min<int64_t>(8, m - r); a.W = wd.p; a.bf16 = bf16; a.n_out = vocab; a.k = k;
                a.Y0 = static_cast<float*>(logits.p); a.ldy0 = vocab;
                hip_check(launch_llm_gemv(a, nullptr), "lm head");
                hip_check(launch_score_rows(a.Y0, vocab, a.rows, vocab, T + r, LP + r, TP + r, TL + r, LS + r, nullptr), "score rows");
            }
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        }
        if (logprob_out) hip_check(hipMemcpy(logprob_out, LP, ob, hipMemcpyDeviceToHost), "D2H logprob");
        if (top_out) hip_check(hipMemcpy(top_out, TP, ob, hipMemcpyDeviceToHost), "D2H top");
        if (top_logprob_out) hip_check(hipMemcpy(top_logprob_out, TL, ob, hipMemcpyDeviceToHost), "D2H top logprob");
        if (lse_out) hip_check(hipMemcpy(lse_out, LS, ob, hipMemcpyDeviceToHost), "D2H lse");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_score_head_topk(int32_t device, const float* hidden, int64_t m, int32_t k, const void* W, int32_t bf16,
                                                            int32_t vocab, const uint32_t* targets, int32_t slab_tiles, int32_t fused,
                                                            int32_t top_k, float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out,
                                                            float* lse_out)
{
    if (!hidden || !W || !targets) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || m > (1 << 20) || k <= 0 || vocab <= 0 || slab_tiles < 0 || (bf16 != 0 && bf16 != 1))
            throw InvalidConfig("invalid score head dimensions");
        if (top_k < 1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > vocab)
            throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [1, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                                "] and not above vocab (" + std::to_string(vocab) + ")");
        if (fused ? k % 32 != 0 : k % 8 != 0) throw InvalidConfig(fused ? "the fused score head needs k % 32 == 0" : "the rows route needs k % 8 == 0");
        for (int64_t r = 0; r < m; ++r)
            if (targets[r] >= (uint32_t)vocab) throw InvalidConfig("targets[" + std::to_string(r) + "] is not below vocab");
        use_device(device);
        if (m == 0) return;
        const size_t xb = (size_t)m * k * 4, wb = (size_t)vocab * k * (bf16 ? 2 : 4), ob = (size_t)m * 4, kb = ob * top_k;
        DeviceBuf xd(xb), wd(wb), td(ob), lp(ob), ti(kb), tl(kb), ls(ob);
        hip_check(hipMemcpy(xd.p, hidden, xb, hipMemcpyHostToDevice), "H2D hidden");
        hip_check(hipMemcpy(wd.p, W, wb, hipMemcpyHostToDevice), "H2D W");
        hip_check(hipMemcpy(td.p, targets, ob, hipMemcpyHostToDevice), "H2D targets");
        const float* X = static_cast<const float*>(xd.p);
        const uint32_t* T = static_cast<const uint32_t*>(td.p);
        float *LP = static_cast<float*>(lp.p), *TL = static_cast<float*>(tl.p), *LS = static_cast<float*>(ls.p);
        uint32_t* TI = static_cast<uint32_t*>(ti.p);
        if (fused) {
            DeviceBuf scratch(score_head_topk_scratch_bytes((int)m, vocab, slab_tiles, top_k));
            hip_check(launch_score_head_topk(X, k, (int)m, wd.p, bf16, vocab, k, T, slab_tiles, top_k, scratch.p, LP, TI, TL, LS, nullptr),
                      "score head top-k");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        } else {
            DeviceBuf logits((size_t)8 * vocab * 4);
            for (int64_t r = 0; r < m; r += 8) {
                LlmGemvArgs a;
                a.X = X + r * k; a.ldx = k; a.rows = (int)std::min<int64_t>(8, m - r); a.W = wd.p; a.bf16 = bf16; a.n_out = vocab; a.k = k;
                a.Y0 = static_cast<float*>(logits.p); a.ldy0 = vocab;
                hip_check(launch_llm_gemv(a, nullptr), "lm head");
                hip_check(launch_score_rows_topk(a.Y0, vocab, a.rows, vocab, T + r, top_k, LP + r, TI + r * top_k, TL + r * top_k, LS + r, nullptr),
                          "score rows top-k");
            }
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        }
        if (logprob_out) hip_check(hipMemcpy(logprob_out, LP, ob, hipMemcpyDeviceToHost), "D2H logprob");
        if (topk_ids_out) hip_check(hipMemcpy(topk_ids_out, TI, kb, hipMemcpyDeviceToHost), "D2H top-k ids");
        if (topk_logprob_out) hip_check(hipMemcpy(topk_logprob_out, TL, kb, hipMemcpyDeviceToHost), "D2H top-k logprob");
        if (lse_out) hip_check(hipMemcpy(lse_out, LS, ob, hipMemcpyDeviceToHost), "D2H lse");
    });
}

KJARNI_EXPORT int32_t kjarni_hip_token_logprob_slabs(int32_t rows, int32_t vocab)
{
    return rows < 1 || rows > kLogprobMaxRows || vocab < 1 ? 0 : token_logprob_slabs(rows, vocab);
}

// The generation log-probability kernels alone (logprob_kernels.h), on logits given by the host: one launcher pair per call over
// logits [calls, rows, ld].  Even calls read the chosen logit from the row itself; odd calls take raw_copy in the slab pass and
// read it from the copy, which must come back as the row's bits.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_token_logprobs(int32_t device, const float* logits, int32_t calls, int32_t rows, int64_t ld,
                                                           int32_t vocab, const int32_t* tokens, int32_t top_k, float* logprob_out,
                                                           uint32_t* topk_ids_out, float* topk_logprob_out, float* lse_out, int32_t* slabs_out)
{
    if (!logits || !tokens || !logprob_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (calls < 0 || calls > 4096 || vocab < 1 || ld < vocab || ld > (1 << 24))
            throw InvalidConfig("invalid token_logprobs dimensions (calls 0 .. 4096, vocab >= 1, ld >= vocab)");
        if (rows < 1 || rows > kLogprobMaxRows) throw InvalidConfig("rows must be 1.." + std::to_string(kLogprobMaxRows));
        if (top_k < 0 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > vocab)
            throw InvalidConfig("top_k (" + std::to_string(top_k) + ") must be in [0, " + std::to_string(KJARNI_SCORE_TOPK_MAX) +
                                "] and not above vocab (" + std::to_string(vocab) + ")");
        const size_t n = (size_t)calls * (size_t)rows;
        for (size_t i = 0; i < n; ++i)
            if (tokens[i] < -1 || tokens[i] >= vocab) throw InvalidConfig("tokens[" + std::to_string(i) + "] is neither -1 nor below vocab");
        use_device(device);
        if (slabs_out) *slabs_out = token_logprob_slabs(rows, vocab);
        if (calls == 0) return;
        const size_t call_floats = (size_t)rows * (size_t)ld, ob = n * 4, kb = std::max<size_t>(ob * (size_t)top_k, 4);
        const auto ld_buf = upload(logits, (size_t)calls * call_floats * 4, "H2D logits");
        const auto tk_buf = upload(tokens, ob, "H2D tokens");
        GuardedBuf lp(ob), ti(kb), tl(kb), ls(ob), scratch(token_logprob_scratch_bytes(rows, vocab)), copy((size_t)rows * (size_t)vocab * 4);
        // what a skipped row must come back as: the caller's own values
        hip_check(hipMemcpy(lp.buf.p, logprob_out, ob, hipMemcpyHostToDevice), "H2D logprob");
        if (topk_ids_out && top_k) hip_check(hipMemcpy(ti.buf.p, topk_ids_out, ob * top_k, hipMemcpyHostToDevice), "H2D top-k ids");
        if (topk_logprob_out && top_k) hip_check(hipMemcpy(tl.buf.p, topk_logprob_out, ob * top_k, hipMemcpyHostToDevice), "H2D top-k logprob");
        if (lse_out) hip_check(hipMemcpy(ls.buf.p, lse_out, ob, hipMemcpyHostToDevice), "H2D lse");
        std::vector<float> back((size_t)rows * (size_t)vocab);
        for (int32_t c = 0; c < calls; ++c) {
            const float* lg = static_cast<const float*>(ld_buf->p) + (size_t)c * call_floats;
            const bool copied = (c & 1) != 0;
            TokenLogprobArgs a;
            a.logits = lg; a.ld = ld; a.rows = rows; a.vocab = vocab; a.top_k = top_k; a.scratch = scratch.buf.p;
            if (copied) { a.raw_copy = copy.as<float>(); a.ld_copy = vocab; }
            TokenLogprobRecord r;
            r.raw = copied ? copy.as<float>() : lg; r.ld_raw = copied ? (int64_t)vocab : ld;
            r.tokens = static_cast<const int32_t*>(tk_buf->p) + (size_t)c * rows;
            r.slots = top_k;
            r.logprob = lp.as<float>() + (size_t)c * rows; r.lse = ls.as<float>() + (size_t)c * rows;
            r.topk_ids = ti.as<uint32_t>() + (size_t)c * rows * top_k; r.topk_logprob = tl.as<float>() + (size_t)c * rows * top_k;
            launcher_check(launch_token_logprob_partial(a, nullptr), "token logprob partial");
            launcher_check(launch_token_logprob_finish(a, r, nullptr), "token logprob finish");
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            if (copied) {
                hip_check(hipMemcpy(back.data(), copy.buf.p, back.size() * 4, hipMemcpyDeviceToHost), "D2H raw copy");
                for (int32_t q = 0; q < rows; ++q)
                    expect(std::memcmp(back.data() + (size_t)q * vocab, logits + (size_t)c * call_floats + (size_t)q * ld, (size_t)vocab * 4) == 0,
                           "token logprobs: the raw copy is not the row");
            }
        }
        lp.check("logprob"); ti.check("top-k ids"); tl.check("top-k logprob"); ls.check("lse"); scratch.check("slab scratch"); copy.check("raw copy");
        hip_check(hipMemcpy(logprob_out, lp.buf.p, ob, hipMemcpyDeviceToHost), "D2H logprob");
        if (topk_ids_out && top_k) hip_check(hipMemcpy(topk_ids_out, ti.buf.p, ob * top_k, hipMemcpyDeviceToHost), "D2H top-k ids");
        if (topk_logprob_out && top_k) hip_check(hipMemcpy(topk_logprob_out, tl.buf.p, ob * top_k, hipMemcpyDeviceToHost), "D2H top-k logprob");
        if (lse_out) hip_check(hipMemcpy(lse_out, ls.buf.p, ob, hipMemcpyDeviceToHost), "D2H lse");
    });
}

// Timing of the pair against the kernel it replaces on the step (tools/bench_more.py llm_logprobs): `iters` launch pairs over
// logits [rows, vocab], and `iters` passes of launch_score_rows_topk over the same rows, 8 at a time, with the rows' own arg-max
// ids as targets.  top_k 1..8.
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_token_logprobs_bench(int32_t device, const float* logits, int32_t rows, int32_t vocab, int32_t top_k,
                                                                 int32_t iters, float* pair_ms_out, float* score_rows_ms_out)
{
    if (!logits || !pair_ms_out || !score_rows_ms_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > kLogprobMaxRows || vocab < 1 || vocab > (1 << 24) || iters < 1 || iters > 100000)
            throw InvalidConfig("rows 1..64, vocab 1..2^24, iters 1..100000");
        if (top_k < 1 || top_k > KJARNI_SCORE_TOPK_MAX || top_k > vocab) throw InvalidConfig("top_k must be 1..8 and not above vocab");
        use_device(device);
        const size_t n = (size_t)rows, kb = n * (size_t)top_k * 4;
        const auto lg = upload(logits, n * (size_t)vocab * 4, "H2D logits");
        GuardedBuf lp(n * 4), ti(kb), tl(kb), scratch(token_logprob_scratch_bytes(rows, vocab)), tg(n * 4);
        hip_check(hipMemset(tg.buf.p, 0, n * 4), "memset targets");
        TokenLogprobArgs a;
        a.logits = static_cast<const float*>(lg->p); a.ld = vocab; a.rows = rows; a.vocab = vocab; a.top_k = top_k; a.scratch = scratch.buf.p;
        TokenLogprobRecord r;
        r.raw = a.logits; r.ld_raw = vocab; r.slots = top_k;
        r.logprob = lp.as<float>(); r.topk_ids = ti.as<uint32_t>(); r.topk_logprob = tl.as<float>();
        time_launches(iters, pair_ms_out, [&] {
            launcher_check(launch_token_logprob_partial(a, nullptr), "token logprob partial");
            launcher_check(launch_token_logprob_finish(a, r, nullptr), "token logprob finish");
        });
        time_launches(iters, score_rows_ms_out, [&] {
            for (int q = 0; q < rows; q += 8) {
                const int m = std::min(8, rows - q);
                launcher_check(launch_score_rows_topk(a.logits + (size_t)q * vocab, vocab, m, vocab, tg.as<uint32_t>() + q, top_k, lp.as<float>() + q,
                                                      ti.as<uint32_t>() + (size_t)q * top_k, tl.as<float>() + (size_t)q * top_k, nullptr, nullptr),
                               "score rows top-k");
            }
        });
        lp.check("logprob"); ti.check("top-k ids"); tl.check("top-k logprob"); scratch.check("slab scratch");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_attention(int32_t device, const float* qkv, const uint32_t* mask,
                                                      int64_t batch, int32_t seq, int32_t heads, int32_t head_dim,
                                                      float mask_value, float* ctx, int32_t iters, float* ms_out)
{
    if (!qkv || !ctx) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (batch < 0 || seq <= 0 || heads <= 0 || head_dim <= 0) throw InvalidConfig("invalid attention dimensions");
        use_device(device);
        if (batch == 0) return;
        const size_t T = (size_t)batch * seq, H = (size_t)heads * head_dim;
        DeviceBuf qd(T * 3 * H * 4), md(T * 4), cd(T * H * 4);
        hip_check(hipMemcpy(qd.p, qkv, T * 3 * H * 4, hipMemcpyHostToDevice), "H2D qkv");
        if (mask) hip_check(hipMemcpy(md.p, mask, T * 4, hipMemcpyHostToDevice), "H2D mask");
        time_launches(iters, ms_out, [&] {
            hip_check(launch_attention((const float*)qd.p, mask ? (const uint32_t*)md.p : nullptr, batch, seq, heads,
                                       head_dim, mask_value, (float*)cd.p, nullptr),
                      "attention");
        });
        hip_check(hipMemcpy(ctx, cd.p, T * H * 4, hipMemcpyDeviceToHost), "D2H ctx");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_attention_biased(int32_t device, const float* qkv, const uint32_t* mask,
                                                             const float* position_bias, int32_t bias_seq, int64_t batch,
                                                             int32_t seq, int32_t heads, int32_t head_dim, int32_t scale_qk,
                                                             float mask_value, float* ctx)
{
    if (!qkv || !ctx) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (batch < 0 || seq <= 0 || heads <= 0 || head_dim <= 0) throw InvalidConfig("invalid attention dimensions");
        if (position_bias && bias_seq < seq) throw InvalidConfig("position bias is smaller than the sequence");
        use_device(device);
        if (batch == 0) return;
        const size_t T = (size_t)batch * seq, H = (size_t)heads * head_dim;
        const size_t bias_bytes = position_bias ? (size_t)heads * bias_seq * bias_seq * 4 : 4;
        DeviceBuf qd(T * 3 * H * 4), md(T * 4), cd(T * H * 4), bd(bias_bytes);
        hip_check(hipMemcpy(qd.p, qkv, T * 3 * H * 4, hipMemcpyHostToDevice), "H2D qkv");
        if (mask) hip_check(hipMemcpy(md.p, mask, T * 4, hipMemcpyHostToDevice), "H2D mask");
        if (position_bias) hip_check(hipMemcpy(bd.p, position_bias, bias_bytes, hipMemcpyHostToDevice), "H2D position bias");
        hip_check(launch_attention_biased((const float*)qd.p, mask ? (const uint32_t*)md.p : nullptr,
                                          position_bias ? (const float*)bd.p : nullptr, bias_seq, batch, seq, heads, head_dim,
                                          scale_qk != 0, mask_value, (float*)cd.p, nullptr),
                  "attention (position bias)");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(ctx, cd.p, T * H * 4, hipMemcpyDeviceToHost), "D2H ctx");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_pool(int32_t device, const float* hidden_states, const uint32_t* mask, int64_t batch,
                                                 int32_t seq, int32_t hidden, KjarniHipPooling pooling, int32_t normalize, float* out)
{
    if (!hidden_states || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (batch < 0 || seq <= 0 || hidden <= 0 || hidden > 1024) throw InvalidConfig("invalid pooling dimensions");
        const PoolMode mode = pool_mode(pooling);   // (throws InvalidConfig for a value outside the enum)
        use_device(device);
        if (batch == 0) return;
        const size_t T = (size_t)batch * seq;
        DeviceBuf hd(T * hidden * 4), md(T * 4), od((size_t)batch * hidden * 4);
        hip_check(hipMemcpy(hd.p, hidden_states, T * hidden * 4, hipMemcpyHostToDevice), "H2D hidden states");
        std::vector<uint32_t> ones;
        if (!mask) ones.assign(T, 1u);
        hip_check(hipMemcpy(md.p, mask ? mask : ones.data(), T * 4, hipMemcpyHostToDevice), "H2D mask");
        hip_check(launch_pool((const float*)hd.p, (const uint32_t*)md.p, batch, seq, hidden, mode, normalize,
                              (float*)od.p, nullptr),
                  "pool");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(out, od.p, (size_t)batch * hidden * 4, hipMemcpyDeviceToHost), "D2H pooled");
    });
}

// ---- the encoder's packed-row kernels, alone --------------------------------------------------------------------------------------
// One launcher call per hook on host arrays.  Every argument is checked before a device is asked for; every output is uploaded as
// the caller gave it and returned whole; a guard band lies behind every device buffer -- checked behind an output, NaN behind an
// input, so that a read past its end poisons the result.

namespace {

// A device copy of `bytes` host bytes with `guard_words` words of the guard pattern (a NaN) behind it.
struct BandBuf {
    static constexpr uint32_t kGuard = GuardedBuf::kGuard;
    size_t bytes, guard_words;
    DeviceBuf buf;
    BandBuf(const void* src, size_t b, size_t guard_words_, const char* what) : bytes((b + 3) / 4 * 4), guard_words(guard_words_), buf(bytes + guard_words_ * 4)
    {
        if (src && b) hip_check(hipMemcpy(buf.p, src, b, hipMemcpyHostToDevice), what);
        hip_check(hipMemsetD32((hipDeviceptr_t)((char*)buf.p + bytes), (int)kGuard, guard_words), "guard band");
    }
    template <class T>
    T* as() const { return static_cast<T*>(buf.p); }
    // the band intact, then the buffer back to the host
    void fetch(void* host, size_t b, const char* what) const
    {
        std::vector<uint32_t> g(guard_words);
        hip_check(hipMemcpy(g.data(), (char*)buf.p + bytes, guard_words * 4, hipMemcpyDeviceToHost), "D2H guard band");
        for (size_t i = 0; i < guard_words; ++i)
            if (g[i] != kGuard) throw std::runtime_error(std::string(what) + ": guard band touched at word " + std::to_string(i));
        if (host && b) hip_check(hipMemcpy(host, buf.p, b, hipMemcpyDeviceToHost), what);
    }
};

static_assert((int)KJARNI_HIP_ATTN_NOTHING == ATTN_NOTHING && (int)KJARNI_HIP_ATTN_SPLIT == ATTN_SPLIT && (int)KJARNI_HIP_ATTN_PIPE_PADDED == ATTN_PIPE_PADDED &&
                  (int)KJARNI_HIP_ATTN_PIPE_PACKED == ATTN_PIPE_PACKED && (int)KJARNI_HIP_ATTN_PIPE_SHORT == ATTN_PIPE_SHORT &&
                  (int)KJARNI_HIP_ATTN_CHUNKED == ATTN_CHUNKED && (int)KJARNI_HIP_ATTN_GENERIC == ATTN_GENERIC, "the header's attention kernels are the launcher's");

constexpr size_t kBandWords = 64;    // behind the small buffers
constexpr int64_t kBandRows = 128;   // behind qkv, ctx and the hidden states: a whole query block / key chunk of rows

// cu [n + 1]: prefix sums of the sentences' lengths from 0; every sentence holds 1 .. max_len rows (the kernels compute extents
// from len - 1 and size their grids by max_len); the last entry at most `rows`.
void check_cu(const int32_t* cu, int64_t n, int32_t max_len, int64_t rows)
{
    if (n < 1 || n > (1 << 20)) throw InvalidConfig("batch must be 1 .. 2^20");
    if (max_len < 1 || max_len > 8192) throw InvalidConfig("the longest sentence must be 1 .. 8192 rows");
    if (cu[0] != 0) throw InvalidConfig("cu[0] must be 0");
    for (int64_t b = 0; b < n; ++b) {
        if (cu[b + 1] <= cu[b])
            throw InvalidConfig("cu[" + std::to_string(b + 1) + "] does not exceed cu[" + std::to_string(b) + "]: sentence " + std::to_string(b) +
                                " is empty or cu decreases");
        if (cu[b + 1] - cu[b] > max_len)
            throw InvalidConfig("sentence " + std::to_string(b) + " is longer than the " + std::to_string(max_len) + " rows the call is sized for");
    }
    if (cu[n] > rows) throw InvalidConfig("cu[batch] = " + std::to_string(cu[n]) + " reaches past the " + std::to_string(rows) + " rows given");
}

void check_mask_shape(int64_t batch, int32_t seq)
{
    if (batch < 1 || batch > (1 << 20) || seq < 1 || seq > (1 << 16) || batch * seq > ((int64_t)1 << 26))
        throw InvalidConfig("batch must be 1 .. 2^20, seq 1 .. 2^16, batch * seq at most 2^26");
}

}  // namespace

// launch_prefill_gemm_fp8 on host arrays: kjarni_hip_op_prefill_gemm's arguments with the weights as FP8 codes [n, k] and their
// scales [scale_rows, scale_cols] (the kind from fp8_scale_kind()).
KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_prefill_gemm_fp8(int32_t device, const float* a, int64_t lda, int32_t a_rows, const void* codes,
                                                             const float* scale, int32_t scale_rows, int32_t scale_cols, const float* bias,
                                                             const float* r, int64_t ldr, int32_t r_is_y, float* y, int64_t ldy, float* gate,
                                                             int32_t m, int32_t n, int32_t k, int32_t split, int32_t* ksplit_used,
                                                             int64_t* scratch_written)
{
    if (!a || !codes || !scale || !y || !ksplit_used) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || m > 4096 || a_rows < std::max(m, 1) || a_rows > 8192) throw InvalidConfig("m must be 0 .. 4096 and a_rows max(m, 1) .. 8192");
        if (n < 1 || k < 1 || n > (1 << 17) || k > (1 << 16) || (int64_t)n * k > ((int64_t)1 << 26))
            throw InvalidConfig("n must be 1 .. 2^17, k 1 .. 2^16, n * k at most 2^26");
        if (k % 32 || lda % 4) throw InvalidConfig("launch_prefill_gemm_fp8 refuses these arguments: k a multiple of 32, lda a multiple of 4");
        if (lda < k || ldy < n || std::max(lda, ldy) > (1 << 18)) throw InvalidConfig("lda must cover k and ldy n (at most 2^18)");
        const bool res = r_is_y || r;
        const int64_t ldr_ = r_is_y ? ldy : ldr;
        if (res && (ldr_ < n || ldr_ > (1 << 18))) throw InvalidConfig("ldr must cover n (at most 2^18)");
        if (gate && (ldy != n || (n & 3))) throw InvalidConfig("launch_prefill_gemm_fp8 refuses these arguments: a gate needs ldy == n and n a multiple of 4");
        if (split != 0 && split != 1) throw InvalidConfig("split must be 0 or 1");
        if (scratch_written && !split) throw InvalidConfig("scratch_written without split");
        const int kind = scale_rows < 1 || scale_cols < 1 ? -1 : fp8_scale_kind(n, k, scale_rows, scale_cols);
        if (kind < 0)
            throw InvalidConfig("FP8 prompt GEMM: a scale of shape [" + std::to_string(scale_rows) + ", " + std::to_string(scale_cols) +
                                "] is neither [1, 1] (per tensor), [n, 1] (per channel) nor [ceil(n / 128), k / 128] (block)");
        const uint8_t* c = static_cast<const uint8_t*>(codes);
        for (int64_t i = 0, e = (int64_t)n * k; i < e; ++i)
            if ((c[i] & 0x7F) == 0x7F) throw InvalidConfig("FP8 prompt GEMM: NaN code at element " + std::to_string(i));
        use_device(device);
        const size_t ab = (size_t)a_rows * (size_t)lda * 4, wb = (size_t)n * (size_t)k, yb = (size_t)m * (size_t)ldy * 4;
        const size_t scb = (size_t)scale_rows * (size_t)scale_cols * 4;
        const size_t rb = r && !r_is_y ? (size_t)m * (size_t)ldr * 4 : 0, gb = gate ? (size_t)m * (size_t)n * 4 : 0;
        const size_t sb = split ? prefill_gemm_scratch_floats(m, n) * 4 : 0;
        BandBuf ad(a, ab, kBandWords, "H2D a"), wd(codes, wb, kBandWords, "H2D codes"), scd(scale, scb, kBandWords, "H2D scales");
        BandBuf bd(bias, bias ? (size_t)n * 4 : 0, kBandWords, "H2D bias"), rd(rb ? r : nullptr, rb, kBandWords, "H2D r");
        BandBuf yd(y, yb, kBandWords, "H2D y"), gd(gate, gb, kBandWords, "H2D gate"), sd(nullptr, sb, kBandWords, "scratch");
        if (sb) hip_check(hipMemset(sd.buf.p, 0xFF, sb), "poison scratch");  // (all-ones words are NaN: a slab the kernels skip would show)
        Fp8Mat W;
        W.n = n; W.k = k; W.codes = wd.as<const uint8_t>(); W.scale = scd.as<const float>(); W.kind = kind;
        const float* bp = bias ? bd.as<const float>() : nullptr;
        const float* rp = r_is_y ? yd.as<const float>() : (r ? rd.as<const float>() : nullptr);
        float* sp = split ? sd.as<float>() : nullptr;
        *ksplit_used = prefill_gemm_launch_ksplit(bp, rp, ldr_, yd.as<const float>(), ldy, m, n, k, sp);
        launcher_check(launch_prefill_gemm_fp8(ad.as<const float>(), lda, W, bp, rp, ldr_, yd.as<float>(), ldy, m, nullptr, sp,
                                               gate ? gd.as<float>() : nullptr), "fp8 prefill gemm");
        hip_check(hipDeviceSynchronize(), "sync");
        yd.fetch(y, yb, "D2H y");
        gd.fetch(gate, gb, "D2H gate");
        sd.fetch(nullptr, 0, "scratch");
        if (scratch_written) {  // the scratch words that no longer hold the poison
            std::vector<uint32_t> words(sb / 4);
            hip_check(hipMemcpy(words.data(), sd.buf.p, sb, hipMemcpyDeviceToHost), "D2H scratch");
            *scratch_written = (int64_t)(words.size() - (size_t)std::count(words.begin(), words.end(), 0xFFFFFFFFu));
        }
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_mask_lengths(int32_t device, const uint32_t* mask, int64_t batch, int32_t seq, uint32_t* lens_out)
{
    if (!mask || !lens_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_mask_shape(batch, seq);
        use_device(device);
        const BandBuf md(mask, (size_t)batch * seq * 4, kBandWords, "H2D mask"), ld(lens_out, (size_t)batch * 4, kBandWords, "H2D lens");
        launcher_check(launch_mask_lengths(md.as<uint32_t>(), batch, seq, ld.as<uint32_t>(), nullptr), "mask_lengths");
        hip_check(hipDeviceSynchronize(), "sync");
        ld.fetch(lens_out, (size_t)batch * 4, "lens");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_pack_index(int32_t device, const uint32_t* mask, const int32_t* cu, int64_t batch, int32_t seq,
                                                       int32_t* tok_src, int32_t capacity)
{
    if (!mask || !cu || !tok_src) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_mask_shape(batch, seq);
        if (capacity < 0 || capacity > (1 << 26)) throw InvalidConfig("capacity must be 0 .. 2^26");
        // the kernel writes tok_src + cu[b] + (rank of the kept token) unchecked: cu must be the prefix sums of the mask's own counts
        if (cu[0] != 0) throw InvalidConfig("cu[0] must be 0");
        for (int64_t b = 0; b < batch; ++b) {
            if (cu[b + 1] < cu[b]) throw InvalidConfig("cu decreases at " + std::to_string(b + 1));
            int32_t kept = 0;
            for (int32_t s = 0; s < seq; ++s) kept += mask[b * seq + s] != 0u;
            if (cu[b + 1] - cu[b] != kept)
                throw InvalidConfig("cu gives sentence " + std::to_string(b) + " " + std::to_string(cu[b + 1] - cu[b]) + " rows, its mask keeps " +
                                    std::to_string(kept));
        }
        if (cu[batch] > capacity) throw InvalidConfig("cu[batch] = " + std::to_string(cu[batch]) + " exceeds the capacity of tok_src");
        use_device(device);
        const BandBuf md(mask, (size_t)batch * seq * 4, kBandWords, "H2D mask"), cd(cu, (size_t)(batch + 1) * 4, kBandWords, "H2D cu");
        const BandBuf td(tok_src, (size_t)capacity * 4, kBandWords, "H2D tok_src");
        launcher_check(launch_pack_index(md.as<uint32_t>(), cd.as<int32_t>(), batch, seq, td.as<int32_t>(), nullptr), "pack_index");
        hip_check(hipDeviceSynchronize(), "sync");
        td.fetch(tok_src, (size_t)capacity * 4, "tok_src");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_encoder_embed(int32_t device, const uint32_t* ids, const uint32_t* type_ids, const float* word,
                                                          const float* pos, const float* type, const float* gamma, const float* beta, float eps,
                                                          int64_t rows, int64_t batch, int32_t seq, int32_t hidden, int32_t vocab, int32_t max_pos,
                                                          int32_t type_vocab, int32_t pos_offset, int32_t scale_embeddings,
                                                          const int32_t* tok_src, float* out)
{
    if (!ids || !word || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_mask_shape(batch, seq);
        const int64_t padded = batch * seq;
        if (rows < 1 || rows > (1 << 22) || hidden < 1 || hidden > 8192 || rows * hidden > ((int64_t)1 << 28))
            throw InvalidConfig("rows must be 1 .. 2^22, hidden 1 .. 8192, rows * hidden at most 2^28");
        if (vocab < 1 || vocab > (1 << 20) || (int64_t)vocab * hidden > ((int64_t)1 << 26)) throw InvalidConfig("vocab must be 1 .. 2^20, vocab * hidden at most 2^26");
        if (!tok_src && rows > padded) throw InvalidConfig("without tok_src row t is token t: rows must not exceed batch * seq");
        if (tok_src)
            for (int64_t t = 0; t < rows; ++t)
                if (tok_src[t] < 0 || tok_src[t] >= padded)
                    throw InvalidConfig("tok_src[" + std::to_string(t) + "] = " + std::to_string(tok_src[t]) + " is outside [0, batch * seq)");
        if (gamma && !beta) throw InvalidConfig("LayerNorm needs beta with gamma");
        if (pos && (max_pos <= 0 || max_pos > (1 << 16))) throw InvalidConfig("pos needs max_pos 1 .. 2^16");
        if (!pos && max_pos < 0) throw InvalidConfig("max_pos must not be negative");
        if (pos_offset < 0 || pos_offset > (1 << 16)) throw InvalidConfig("pos_offset must be 0 .. 2^16");
        if (type && (type_vocab < 1 || type_vocab > 4096)) throw InvalidConfig("type needs type_vocab 1 .. 4096");
        if (type && type_ids)  // (the kernel clamps them; the reference panics: the host validates, rowops.hip)
            for (int64_t i = 0; i < padded; ++i)
                if (type_ids[i] >= (uint32_t)type_vocab)
                    throw InvalidConfig("type_ids[" + std::to_string(i) + "] = " + std::to_string(type_ids[i]) + " is not below type_vocab");
        use_device(device);
        const size_t hb = (size_t)hidden * 4;
        const BandBuf idd(ids, (size_t)padded * 4, kBandWords, "H2D ids"), tyd(type_ids, type_ids ? (size_t)padded * 4 : 0, kBandWords, "H2D type_ids");
        const BandBuf wd(word, (size_t)vocab * hb, kBandWords, "H2D word"), pd(pos, pos ? (size_t)max_pos * hb : 0, kBandWords, "H2D pos");
        const BandBuf td(type, type ? (size_t)type_vocab * hb : 0, kBandWords, "H2D type"), gd(gamma, gamma ? hb : 0, kBandWords, "H2D gamma");
        const BandBuf bd(beta, beta ? hb : 0, kBandWords, "H2D beta"), sd(tok_src, tok_src ? (size_t)rows * 4 : 0, kBandWords, "H2D tok_src");
        const BandBuf od(out, (size_t)rows * hb, (size_t)kBandRows * hidden, "H2D out");
        launcher_check(launch_embed_layernorm(idd.as<uint32_t>(), type_ids ? tyd.as<uint32_t>() : nullptr, wd.as<float>(), pos ? pd.as<float>() : nullptr,
                                              type ? td.as<float>() : nullptr, gamma ? gd.as<float>() : nullptr, beta ? bd.as<float>() : nullptr, eps,
                                              rows, seq, hidden, vocab, max_pos, type_vocab, pos_offset, scale_embeddings ? 1 : 0, od.as<float>(),
                                              nullptr, tok_src ? sd.as<int32_t>() : nullptr), "embed");
        hip_check(hipDeviceSynchronize(), "sync");
        od.fetch(out, (size_t)rows * hb, "out");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_encoder_rope(int32_t device, float* qkv, const float* cos_t, const float* sin_t, int64_t rows,
                                                         int32_t seq, int32_t heads, int32_t head_dim, const int32_t* tok_src)
{
    if (!qkv || !cos_t || !sin_t) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (head_dim < 2 || head_dim > 256 || (head_dim & 1) || heads < 1 || heads > 1024) throw InvalidConfig("head_dim must be even, 2 .. 256; heads 1 .. 1024");
        if (seq < 1 || seq > (1 << 16)) throw InvalidConfig("seq must be 1 .. 2^16");
        const int64_t width = 3 * (int64_t)heads * head_dim;
        if (rows < 1 || rows > (1 << 22) || rows * width > ((int64_t)1 << 28)) throw InvalidConfig("rows must be 1 .. 2^22, rows * 3 hidden at most 2^28");
        // the position of row t is tok_src[t] % seq (t % seq without tok_src): a negative entry would read in front of the tables
        if (tok_src)
            for (int64_t t = 0; t < rows; ++t)
                if (tok_src[t] < 0) throw InvalidConfig("tok_src[" + std::to_string(t) + "] is negative");
        use_device(device);
        const size_t tb = (size_t)seq * head_dim * 4, qb = (size_t)rows * width * 4;
        const BandBuf cd(cos_t, tb, kBandWords, "H2D cos"), snd(sin_t, tb, kBandWords, "H2D sin"), sd(tok_src, tok_src ? (size_t)rows * 4 : 0, kBandWords, "H2D tok_src");
        const BandBuf qd(qkv, qb, (size_t)width, "H2D qkv");
        launcher_check(launch_rope_qk(qd.as<float>(), cd.as<float>(), snd.as<float>(), rows, seq, heads, head_dim, nullptr,
                                      tok_src ? sd.as<int32_t>() : nullptr), "rope");
        hip_check(hipDeviceSynchronize(), "sync");
        qd.fetch(qkv, qb, "qkv");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_attention_route(int64_t batch, int32_t seq_or_max_len, int32_t heads, int32_t head_dim, int32_t aligned,
                                                         int32_t packed, int32_t* route_out)
{
    if (!route_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (heads < 1 || head_dim < 1 || heads > (1 << 16) || head_dim > (1 << 16) || batch > ((int64_t)1 << 32))
            throw InvalidConfig("heads and head_dim must be 1 .. 2^16, batch at most 2^32");
        const AttentionRoute r = attention_route(batch, seq_or_max_len, heads, head_dim, aligned != 0, packed != 0);
        route_out[0] = (int32_t)r.kernel;
        route_out[1] = (int32_t)r.grid;
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_attention_packed(int32_t device, const float* qkv, const int32_t* cu, int64_t batch, int32_t max_len,
                                                             int32_t heads, int32_t head_dim, float mask_value, float* ctx, int64_t buffer_rows,
                                                             int32_t* route_out)
{
    if (!qkv || !cu || !ctx || !route_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (heads < 1 || heads > 1024 || head_dim < 1 || head_dim > 256) throw InvalidConfig("heads must be 1 .. 1024, head_dim 1 .. 256");
        const int64_t H = (int64_t)heads * head_dim;
        if (buffer_rows < 1 || buffer_rows > (1 << 22) || (buffer_rows + kBandRows) * 3 * H > ((int64_t)1 << 28))
            throw InvalidConfig("buffer_rows must be 1 .. 2^22, (buffer_rows + 128) * 3 hidden at most 2^28");
        check_cu(cu, batch, max_len, buffer_rows);
        // (hipMalloc returns 256-byte aligned blocks: `aligned` is the hidden width's alone)
        const AttentionRoute route = attention_route(batch, max_len, heads, head_dim, H % 4 == 0, true);
        use_device(device);
        const size_t qb = (size_t)buffer_rows * 3 * H * 4, cb = (size_t)buffer_rows * H * 4;
        const BandBuf qd(qkv, qb, (size_t)kBandRows * 3 * H, "H2D qkv"), cd(cu, (size_t)(batch + 1) * 4, kBandWords, "H2D cu");
        const BandBuf od(ctx, cb, (size_t)kBandRows * H, "H2D ctx");
        launcher_check(launch_attention(qd.as<float>(), nullptr, batch, max_len, heads, head_dim, mask_value, od.as<float>(), nullptr, cd.as<int32_t>()),
                       "attention (packed rows)");
        hip_check(hipDeviceSynchronize(), "sync");
        od.fetch(ctx, cb, "ctx");
        route_out[0] = (int32_t)route.kernel;
        route_out[1] = (int32_t)route.grid;
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_pool_packed(int32_t device, const float* hidden_states, const int32_t* cu, int64_t batch, int32_t seq,
                                                        int32_t hidden, KjarniHipPooling pooling, int32_t normalize, float* out)
{
    if (!hidden_states || !cu || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (hidden < 1 || hidden > 1024) throw InvalidConfig("hidden must be 1 .. 1024");
        const PoolMode mode = pool_mode(pooling);   // (throws InvalidConfig for a value outside the enum)
        check_cu(cu, batch, seq, (int64_t)1 << 22);
        use_device(device);
        const size_t hb = (size_t)cu[batch] * hidden * 4, ob = (size_t)batch * hidden * 4;
        const BandBuf hd(hidden_states, hb, (size_t)kBandRows * hidden, "H2D hidden states"), cd(cu, (size_t)(batch + 1) * 4, kBandWords, "H2D cu");
        const BandBuf od(out, ob, (size_t)4 * hidden, "H2D out");
        launcher_check(launch_pool(hd.as<float>(), nullptr, batch, seq, hidden, mode, normalize ? 1 : 0, od.as<float>(), nullptr, cd.as<int32_t>()),
                       "pool (packed rows)");
        hip_check(hipDeviceSynchronize(), "sync");
        od.fetch(out, ob, "out");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_small_linear(int32_t device, const float* feat, int64_t ld, const float* w, const float* bias,
                                                         int64_t rows, int32_t k, int32_t n, float* out)
{
    if (!feat || !w || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > (1 << 20) || k < 1 || k > (1 << 16) || n < 1 || n > 4096 || ld < k || ld > (1 << 20) || rows * ld > ((int64_t)1 << 28))
            throw InvalidConfig("rows must be 1 .. 2^20, k 1 .. 2^16, n 1 .. 4096, ld k .. 2^20, rows * ld at most 2^28");
        use_device(device);
        const size_t ob = (size_t)rows * n * 4;
        const BandBuf fd(feat, (size_t)rows * ld * 4, kBandWords, "H2D feat"), wd(w, (size_t)n * k * 4, kBandWords, "H2D w");
        const BandBuf bd(bias, bias ? (size_t)n * 4 : 0, kBandWords, "H2D bias"), od(out, ob, kBandWords, "H2D out");
        launcher_check(launch_small_linear(fd.as<float>(), ld, wd.as<float>(), bias ? bd.as<float>() : nullptr, rows, k, n, od.as<float>(), nullptr),
                       "small_linear");
        hip_check(hipDeviceSynchronize(), "sync");
        od.fetch(out, ob, "out");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_row_softmax(int32_t device, const float* in, int64_t rows, int32_t n, int32_t sigmoid, float* out)
{
    if (!in || !out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 1 || rows > (1 << 20) || n < 1 || n > 4096 || rows * n > ((int64_t)1 << 26)) throw InvalidConfig("rows must be 1 .. 2^20, n 1 .. 4096");
        use_device(device);
        const size_t b = (size_t)rows * n * 4;
        const BandBuf id(in, b, kBandWords, "H2D in"), od(out, b, kBandWords, "H2D out");
        launcher_check(launch_row_softmax(id.as<float>(), rows, n, sigmoid ? 1 : 0, od.as<float>(), nullptr), "row_softmax");
        hip_check(hipDeviceSynchronize(), "sync");
        od.fetch(out, b, "out");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_layer_norm(int32_t device, const float* x, const float* gamma,
                                                       const float* beta, float eps, int64_t rows, int32_t hidden,
                                                       float* y, int32_t iters, float* ms_out)
{
    if (!x || !gamma || !beta || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (rows < 0 || hidden <= 0) throw InvalidConfig("invalid LayerNorm dimensions");
        use_device(device);
        if (rows == 0) return;
        const size_t b = (size_t)rows * hidden * 4;
        DeviceBuf xd(b), gd((size_t)hidden * 4), bd((size_t)hidden * 4), yd(b);
        hip_check(hipMemcpy(xd.p, x, b, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(gd.p, gamma, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(bd.p, beta, (size_t)hidden * 4, hipMemcpyHostToDevice), "H2D beta");
        time_launches(iters, ms_out, [&] {
            hip_check(launch_layernorm((const float*)xd.p, (const float*)gd.p, (const float*)bd.p, eps, rows, hidden,
                                       (float*)yd.p, nullptr),
                      "layernorm");
        });
        hip_check(hipMemcpy(y, yd.p, b, hipMemcpyDeviceToHost), "D2H y");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_linear_layer_norm(int32_t device, const float* x, const float* w,
                                                              const float* bias, const float* residual, const float* gamma,
                                                              const float* beta, float eps, int64_t m, int32_t k, int32_t n,
                                                              float* y, int32_t iters, float* ms_out)
{
    if (!x || !w || !residual || !gamma || !beta || !y) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (m < 0 || k <= 0 || n <= 0) throw InvalidConfig("invalid GEMM dimensions");
        use_device(device);
        if (m == 0) return;
        const size_t xb = (size_t)m * k * 4, wb = (size_t)n * k * 4, yb = (size_t)m * n * 4, nb = (size_t)n * 4;
        DeviceBuf xd(xb), wd(wb), bd(nb), rd(yb), gd(nb), ed(nb), yd(yb);
        hip_check(hipMemcpy(xd.p, x, xb, hipMemcpyHostToDevice), "H2D x");
        hip_check(hipMemcpy(wd.p, w, wb, hipMemcpyHostToDevice), "H2D w");
        if (bias) hip_check(hipMemcpy(bd.p, bias, nb, hipMemcpyHostToDevice), "H2D bias");
        const float* bias_d = bias ? (const float*)bd.p : nullptr;
        hip_check(hipMemcpy(rd.p, residual, yb, hipMemcpyHostToDevice), "H2D residual");
        hip_check(hipMemcpy(gd.p, gamma, nb, hipMemcpyHostToDevice), "H2D gamma");
        hip_check(hipMemcpy(ed.p, beta, nb, hipMemcpyHostToDevice), "H2D beta");
        const size_t sf = gemm_scratch_floats(m, n);
        DeviceBuf sd(sf * 4);
        const GemmScratch sc{(float*)sd.p, sf};
        const bool fused = gemm_residual_layernorm_supported(n, k) || gemm_mid_layernorm_supported(m, n, k);
        time_launches(iters, ms_out, [&] {
            if (fused) {
                hip_check(launch_gemm_residual_layernorm((const float*)xd.p, k, (const float*)wd.p, bias_d,
                                                         (const float*)rd.p, n, (const float*)gd.p, (const float*)ed.p, eps,
                                                         (float*)yd.p, n, m, n, k, nullptr, sc),
                          "gemm + layernorm");
            } else {
                hip_check(launch_gemm((const float*)xd.p, k, (const float*)wd.p, bias_d, (const float*)rd.p, n,
                                      (float*)yd.p, n, m, n, k, EPI_BIAS_RESIDUAL, nullptr, sc),
                          "gemm");
                hip_check(launch_layernorm((const float*)yd.p, (const float*)gd.p, (const float*)ed.p, eps, m, n, (float*)yd.p,
                                           nullptr),
                          "layernorm");
            }
        });
        hip_check(hipMemcpy(y, yd.p, yb, hipMemcpyDeviceToHost), "D2H y");
    });
}

// ---- cosine scan ----------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_cosine_scores(int32_t device, const float* queries_dev,
                                                       int32_t n_queries, const float* corpus_dev,
                                                       int64_t n_docs, int32_t dim, KjarniHipCosineMode mode,
                                                       float* scores_out_dev, void* stream)
{
    if (!queries_dev || !corpus_dev || !scores_out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (dim <= 0 || n_queries < 0 || n_docs < 0) throw InvalidConfig("invalid scan dimensions");
        use_device(device);
        hip_check(launch_cosine_scores(queries_dev, n_queries, corpus_dev, n_docs, dim, (int)mode,
                                       scores_out_dev, static_cast<hipStream_t>(stream)),
                  "cosine_scores");
    });
}

KJARNI_EXPORT size_t kjarni_hip_cosine_topk_workspace_bytes(int32_t n_queries, int64_t n_docs, int32_t k)
{
    if (n_queries <= 0 || n_docs <= 0 || k <= 0) return 256;
    return cosine_topk_workspace_bytes(n_queries, n_docs, k);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_cosine_topk(int32_t device, const float* scores_dev, int32_t n_queries,
                                                     int64_t n_docs, int32_t k, void* workspace_dev,
                                                     int64_t* idx_out_dev, float* score_out_dev, void* stream)
{
    if (!scores_dev || !workspace_dev || !idx_out_dev || !score_out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(launch_cosine_topk(scores_dev, n_queries, n_docs, k, workspace_dev, idx_out_dev,
                                     score_out_dev, static_cast<hipStream_t>(stream)),
                  "cosine_topk");
    });
}

KJARNI_EXPORT size_t kjarni_hip_cosine_search_workspace_bytes(int32_t n_queries, int64_t n_docs, int32_t dim, int32_t k)
{
    if (n_queries <= 0 || n_docs <= 0 || k <= 0 || dim <= 0) return 256;
    return cosine_search_workspace_bytes(n_queries, n_docs, dim, k);
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_cosine_search(int32_t device, const float* queries_dev, int32_t n_queries,
                                                       const float* corpus_dev, int64_t n_docs, int32_t dim,
                                                       KjarniHipCosineMode mode, int32_t k, void* workspace_dev,
                                                       int64_t* idx_out_dev, float* score_out_dev, void* stream)
{
    if (!queries_dev || !corpus_dev || !workspace_dev || !idx_out_dev || !score_out_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (dim <= 0 || n_queries < 0 || n_docs < 0 || k < 0) throw InvalidConfig("invalid search dimensions");
        use_device(device);
        hip_check(launch_cosine_search(queries_dev, n_queries, corpus_dev, n_docs, dim, (int)mode, k, workspace_dev, idx_out_dev,
                                       score_out_dev, (hipStream_t)stream),
                  "cosine_search");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_cosine_search_host(int32_t device, const float* queries,
                                                            int32_t n_queries, const float* corpus,
                                                            int64_t n_docs, int32_t dim, KjarniHipCosineMode mode,
                                                            int32_t k, int64_t* idx_out, float* score_out,
                                                            int64_t* n_hits_out)
{
    if (!queries || !corpus || !idx_out || !score_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (dim <= 0 || n_queries < 0 || n_docs < 0 || k < 0) throw InvalidConfig("invalid search dimensions");
        if (n_hits_out) *n_hits_out = 0;
        if (n_queries == 0 || n_docs == 0 || k == 0) return;
        use_device(device);
        const size_t qb = (size_t)n_queries * dim * 4, cb = (size_t)n_docs * dim * 4;
        DeviceBuf q_d(qb), c_d(cb);
        DeviceBuf ws(cosine_search_workspace_bytes(n_queries, n_docs, dim, k));
        DeviceBuf i_d((size_t)n_queries * k * 8), o_d((size_t)n_queries * k * 4);
        hip_check(hipMemcpy(q_d.p, queries, qb, hipMemcpyHostToDevice), "H2D queries");
        hip_check(hipMemcpy(c_d.p, corpus, cb, hipMemcpyHostToDevice), "H2D corpus");
        hip_check(launch_cosine_search((const float*)q_d.p, n_queries, (const float*)c_d.p, n_docs, dim, (int)mode, k, ws.p,
                                       (int64_t*)i_d.p, (float*)o_d.p, nullptr),
                  "cosine_search");
        hip_check(hipMemcpy(idx_out, i_d.p, (size_t)n_queries * k * 8, hipMemcpyDeviceToHost), "D2H idx");
        hip_check(hipMemcpy(score_out, o_d.p, (size_t)n_queries * k * 4, hipMemcpyDeviceToHost), "D2H scores");
        if (mode == KJARNI_HIP_COSINE_SEGMENT) {
            // segment.rs:313-317: a query whose norm is < 1e-9 has no hits.
            for (int32_t j = 0; j < n_queries; ++j) {
                float s2 = 0.0f;
                for (int32_t i = 0; i < dim; ++i) s2 += queries[(size_t)j * dim + i] * queries[(size_t)j * dim + i];
                if (std::sqrt(s2) < 1e-9f)
                    for (int32_t i = 0; i < k; ++i) {
                        idx_out[(size_t)j * k + i] = -1;
                        score_out[(size_t)j * k + i] = -std::numeric_limits<float>::infinity();
                    }
            }
        }
        if (n_hits_out) *n_hits_out = (k < n_docs) ? k : n_docs;
    });
}

// ---- device memory helpers ------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_malloc(int32_t device, size_t bytes, void** out_dev)
{
    if (!out_dev) return KJARNI_ERROR_NULL_POINTER;
    *out_dev = nullptr;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(hipMalloc(out_dev, bytes ? bytes : 4), "hipMalloc");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_free(int32_t device, void* ptr_dev)
{
    if (!ptr_dev) return KJARNI_OK;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(hipFree(ptr_dev), "hipFree");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_memcpy_h2d(int32_t device, void* dst_dev, const void* src, size_t bytes)
{
    if (!dst_dev || !src) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(hipMemcpy(dst_dev, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_memcpy_d2h(int32_t device, void* dst, const void* src_dev, size_t bytes)
{
    if (!dst || !src_dev) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost), "hipMemcpy D2H");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_synchronize(int32_t device)
{
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        use_device(device);
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    });
}
