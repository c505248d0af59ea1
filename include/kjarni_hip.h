/*
 * kjarni_hip.h -- token-level C ABI of the MI355X encoder core.
 *
 * These entry points sit at the reference's token-level boundary
 *   EncoderLanguageModel::get_hidden_states_batch_from_ids
 *     (crates/kjarni-transformers/src/cpu/encoder/traits.rs:66-139)
 *   CpuEncoderOps::forward_tokens (traits.rs:295-313)
 *   SentenceEncoder::encode_batch_flat
 *     (crates/kjarni-models/src/models/sentence_encoder/model.rs:201-218)
 *   CrossEncoder::predict_pairs / SequenceClassifier::predict_logits
 *     (models/cross_encoder/model.rs:170-240, models/sequence_classifier/mod.rs:265-346)
 *   VectorStore::search / Segment::search_vectors
 *     (crates/kjarni-search/src/vector.rs:150-166, crates/kjarni-rag/src/segment.rs:307-337)
 * i.e. the place where the reference's wgpu backend plugs in
 * (GpuEncoderOps, traits.rs:443-527).  The string-level kjarni-ffi surface
 * (kjarni.h) is built on top of them.
 *
 * Plain C: pointers and sizes only.  "_dev" arguments are device pointers on
 * the encoder's HIP device; work is enqueued on `stream` (a hipStream_t passed
 * as void*, NULL = the default stream) and NOT synchronised unless stated.
 * ids / attention mask / token type ids are uint32 [batch, seq] row-major, as
 * in the reference (Array2<u32>).
 */
#ifndef KJARNI_HIP_H
#define KJARNI_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "kjarni.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct KjarniHipEncoder KjarniHipEncoder;

/* Pooling strategies: crates/kjarni-transformers/src/cpu/encoder/config.rs (PoolingStrategy). */
typedef enum KjarniHipPooling {
    KJARNI_HIP_POOL_MEAN = 0,
    KJARNI_HIP_POOL_CLS = 1,
    KJARNI_HIP_POOL_MAX = 2,
    KJARNI_HIP_POOL_LAST_TOKEN = 3,
} KjarniHipPooling;

/* Padding-mask fill value.  The reference overwrites masked scores with -1e9 on
 * its alloc path (utils/masks.rs:4-36) and with -inf on its no-alloc path
 * (cpu/encoder/encoder_self_attention.rs:311-325); AUTO applies its selection
 * rule (cpu/strategy.rs:43-44: no-alloc iff tokens <= 1 or tokens >= 1000) for
 * embed/hidden_states and the alloc value for logits (forward_tokens always
 * takes the alloc path). */
typedef enum KjarniHipMaskFill {
    KJARNI_HIP_MASK_AUTO = 0,
    KJARNI_HIP_MASK_NEG_1E9 = 1,
    KJARNI_HIP_MASK_NEG_INF = 2,
} KjarniHipMaskFill;

/* Number of visible HIP devices (0 when none / no runtime). */
int32_t kjarni_hip_device_count(void);

/* Load <model_dir>/{config.json, model.safetensors} onto HIP device `device`.
 * Errors: KJARNI_ERROR_GPU_UNAVAILABLE (no device), KJARNI_ERROR_MODEL_NOT_FOUND
 * (files missing), KJARNI_ERROR_LOAD_FAILED (bad files). */
KjarniErrorCode kjarni_hip_encoder_load(const char* model_dir, int32_t device, KjarniHipEncoder** out);
void kjarni_hip_encoder_free(KjarniHipEncoder* enc);

int32_t kjarni_hip_encoder_hidden_size(const KjarniHipEncoder* enc);
int32_t kjarni_hip_encoder_num_layers(const KjarniHipEncoder* enc);
int32_t kjarni_hip_encoder_max_seq_len(const KjarniHipEncoder* enc);
int32_t kjarni_hip_encoder_vocab_size(const KjarniHipEncoder* enc);
int32_t kjarni_hip_encoder_num_labels(const KjarniHipEncoder* enc); /* 0: no classification head */
int32_t kjarni_hip_encoder_device(const KjarniHipEncoder* enc);
/* Tokens processed per internal chunk (workspace size); 0 keeps the default. */
KjarniErrorCode kjarni_hip_encoder_set_chunk_tokens(KjarniHipEncoder* enc, int64_t tokens);
/* Ragged batches: embed / logits run the layers over the kept tokens only (mask != 0) when a call has padding, every
 * sentence keeps its token 0 and the mask holds only 0 / 1 -- a padded token is observable through neither output
 * (pooling skips it, pooling/mod.rs:11-33; as a key its score is overwritten, utils/masks.rs:4-36).  Results agree with the
 * padded layout to rounding (<= 1e-6).  `on`:
 *   0  never: every call takes the padded layout (what hidden_states always does);
 *   1  (default) the host-pointer entry points (..._host, and everything built on them: the string-level handles, groups),
 *      whose mask is already on the host -- the device-pointer entry points stay "enqueued on `stream`, never synchronised",
 *      graph-capturable, on the padded layout;
 *   2  the device-pointer embed / logits too: a call of more than one sentence then reads 4 bytes per sentence back and
 *      SYNCHRONISES `stream` once before the layers are enqueued (it blocks the calling thread behind whatever the stream
 *      holds; on a capturing stream the call falls back to the padded layout).  Opt in when ragged device-resident batches
 *      matter more than asynchrony (1.76 x on lengths U{16..128}). */
KjarniErrorCode kjarni_hip_encoder_set_packing(KjarniHipEncoder* enc, int32_t on);

/* Concurrent small calls on one handle -- OPT-IN, default off.  The reference serialises nothing on a handle
 * (kjarni-ffi/src/lib.rs:25-32) and gives every call its own deterministic result; so does this library by default: N threads
 * that each embed or classify one sentence run N independent forwards (on up to four workspaces / streams at once), each
 * bit-identical to the same call made alone.  A single-sentence forward is ~45 dependent launches on a fraction of the chip,
 * so a service that prefers throughput over bit-reproducibility can turn COMBINING on (1 here, or KJARNI_HIP_COMBINE=1 in the
 * environment for every handle the process loads, the string-level handles and groups included): small host-pointer calls
 * (<= 8 rows, <= 1 024 tokens) that arrive while another small call of the same kind is on the device then ride along with the
 * next leader as ONE packed batch (16 threads: 9.7 k -> 28 k encodes/s).  A call that finds the handle idle still runs at once.
 * What it costs: a combined call's result equals the solo call's to rounding (<= 1e-6: the rows take the packed layout and
 * possibly another tile route), not bit for bit, and WHICH calls share a forward depends on arrival times.  If a shared
 * forward fails, each of its calls is run again alone, so only the call that fails by itself reports an error. */
KjarniErrorCode kjarni_hip_encoder_set_combining(KjarniHipEncoder* enc, int32_t on);

/* Mid-size host-pointer calls (2 304 .. 24 576 kept tokens: the reference's default batch of 32 sentences and a few of them)
 * run as two or three parts on as many workspaces / streams, the other parts enqueued by helper threads of the handle: one
 * part's launch gaps, prologues and output bursts fall under the others' matrix work (32 / 48 / 72 / 96 / 160 x 128 tokens: 1.02 /
 * 1.57 / 2.35 / 2.68 / 4.54 -> 0.89 / 1.36 / 1.99 / 2.47 / 3.93 ms).  Sentences are independent.  Up to 8 192 tokens the parts take the
 * projection route the whole call would, so results are bit-identical to the unsplit call (and a call that finds the helpers
 * busy runs unsplit); above that the unsplit call would take the large-batch kernels, the two forms agree to rounding
 * (<= 1e-6), and the split form is what the call computes whenever this is on (deterministically: a part whose helper is busy
 * runs on the caller's thread).  On by default; 0 (or environment KJARNI_HIP_TWO_LANES=0) runs every call as one launch
 * sequence. */
KjarniErrorCode kjarni_hip_encoder_set_two_lanes(KjarniHipEncoder* enc, int32_t on);

/* Opt-in, process-wide, default OFF (or environment KJARNI_HIP_F32_ON_BF16=1, read once at the first projection): the
 * projections of calls above the few-rows range (more than 256 token rows; 128 for models wider than 512) compute their f32
 * products on the bf16 matrix cores.  Every
 * f32 operand is split EXACTLY into three bf16 pieces (8 + 8 + 8 significand bits) on its way into LDS and six of the nine
 * cross products are accumulated in f32 -- the three dropped ones are below 2^-24 of a product, f32's own rounding --
 * so inputs, outputs and the error level are those of f32 arithmetic (measured against float64: the same 2-4e-6 as the f32
 * MFMA kernels, tests/test_gpu_split.py), at 1.1-1.3x their speed (the reference's default batch of 32 sentences x 128
 * tokens: 1.12 -> 0.94 ms per call).  Differences: sums run in another
 * order (results equal to the default path to rounding, not bit for bit), and NON-FINITE inputs: an element that is +-inf or NaN
 * turns every product it takes part in into NaN (the split computes x - bf16(x), and inf - inf is NaN) where the default
 * path keeps an infinity an infinity (inf * finite = inf); finite inputs whose products overflow behave the same in both.  The reference computes in f32
 * (kjarni-transformers/src/linear_layer/linear_layer.rs:160-282); whether f32 results assembled from bf16 pieces meet a
 * deployment's precision policy is the integrator's decision, hence off by default.  Returns the previous setting. */
int32_t kjarni_hip_set_f32_on_bf16(int32_t on);
int32_t kjarni_hip_get_f32_on_bf16(void);

/* Self-test (no counterpart in the reference): the kernels' cross-lane sums and maxima avoid the LDS crossbar (csrc/device_utils.h:
 * v_permlane32_swap / v_permlane16_swap and DPP row rotations in place of ds_bpermute_b32) and claim the `__shfl_xor` butterfly's
 * values bit for bit; this runs every such form against the butterfly it replaces on `waves` x 64 pseudo-random values of
 * seed `seed` (1 .. 4 194 304 waves) and writes the number of lanes that differ to *mismatches_out (0 = the claim holds). */
KjarniErrorCode kjarni_hip_selftest_reductions(int32_t device, uint32_t waves, uint32_t seed, uint32_t* mismatches_out);

/* Measurement aid (bench.py's `clock_ghz` fields; no counterpart in the reference): enqueues ONE wave on `stream` that reads the
 * shader-cycle counter and the constant 100 MHz counter either side of a spin of `spin_us` microseconds (0 = 20; at most
 * 10 000) and writes out_dev[0] = shader cycles, out_dev[1] = 10 ns ticks.  out_dev[0] / out_dev[1] / 10 is the shader clock in
 * GHz the chip holds at that point of the stream -- what a power-limited run lowers while a short one does not.  Asynchronous;
 * out_dev is a device pointer to two uint64. */
KjarniErrorCode kjarni_hip_clock_probe(uint64_t* out_dev, uint32_t spin_us, void* stream);
/* The same reading over `samples` consecutive windows of `window_us` microseconds (1 .. 4096 windows of 10 .. 1 000 000 us, at
 * most ten seconds per launch): out_dev[2 s] = shader cycles, out_dev[2 s + 1] = 10 ns ticks of window s.  Enqueued on a stream
 * of its OWN beside the work being measured (one wave, asleep between its reads) it is the clock the chip holds UNDER that work:
 * f32 matrix-core kernels run the board at its power cap and the clock it settles at there -- not the 2.4 GHz of the data sheet
 * -- is what their rate is a fraction of.  A probe between two kernels of the busy stream reads an idle chip's clock instead. */
KjarniErrorCode kjarni_hip_clock_trace(uint64_t* out_dev, uint32_t samples, uint32_t window_us, void* stream);
/* A non-blocking stream of the library's own for such readings (one per process, made on first use on the current device, never
 * destroyed; NULL if it cannot be made).  hipStreamSynchronize / a later blocking copy from out_dev orders the caller behind it. */
void* kjarni_hip_measurement_stream(void);
/* Waits for it and destroys it (the next kjarni_hip_measurement_stream() makes a new one).  A process has a handful of hardware
 * queues and HIP deals its streams over them: release the stream once the readings are in, or one of an encoder's own streams may
 * share a queue with it. */
void kjarni_hip_measurement_stream_release(void);

/* Thread safety (every entry point of a KjarniHipEncoder / KjarniHipEncoderGroup, device- and host-pointer forms):
 * calls may be made concurrently from any number of host threads and on any streams, as on the reference's
 * handles (its model types are Send + Sync, crates/kjarni-ffi/src/lib.rs:25-32).  The weights are immutable; each
 * call leases one of up to 4 activation workspaces of the handle (a fifth concurrent call waits for a lease),
 * and a workspace that moves from one stream to another is ordered by an event.  Device-pointer forms only
 * ENQUEUE on `stream` (NULL = the legacy default stream); host-pointer forms run on a stream of their own and
 * return when the result is in the caller's buffer.  The profiler (profile_begin / _end) is single-caller.
 *
 * What a sentence's result depends on.  Sentences never influence each other's VALUES beyond rounding, and within one kernel
 * route a row's result is bit-identical whatever shares its call (tests/test_gpu_large_batch.py, test_gpu_encoder.py).  The
 * route, however, follows the call's size -- projections: up to 256 rows / 257 .. 8 192 / more; attention: up to 128
 * (sentence, head) items / more; pooling: calls below 2 048 sentences / more; packed or padded layout -- and every route sums
 * in its own order, so the same sentence in calls of different sizes (or combined with other callers' sentences, below)
 * agrees to rounding (measured <= 1e-6 on unit-norm embeddings), not bit for bit.  The reference makes the same kind of
 * choice by size (linear_layer.rs:164-173: row-vector kernel below 1 000 rows, 4 x 3 block kernel above).
 *
 * hidden_out_dev: f32 [batch, seq, hidden].  type_ids_dev may be NULL (token
 * type row 0 is added to every token, cpu/embeddings/mod.rs:216-223). */
KjarniErrorCode kjarni_hip_encoder_hidden_states(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                                 const uint32_t* mask_dev, const uint32_t* type_ids_dev,
                                                 int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                                 float* hidden_out_dev, void* stream);

/* out_dev: f32 [batch, hidden].  mean-pool + normalize = encode_batch_flat. */
KjarniErrorCode kjarni_hip_encoder_embed(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                         const uint32_t* mask_dev, const uint32_t* type_ids_dev,
                                         int64_t batch, int32_t seq, KjarniHipPooling pooling,
                                         int32_t normalize, KjarniHipMaskFill fill, float* out_dev,
                                         void* stream);

/* logits_out_dev: f32 [batch, num_labels] (rerank score = column 0). */
KjarniErrorCode kjarni_hip_encoder_logits(KjarniHipEncoder* enc, const uint32_t* ids_dev,
                                          const uint32_t* mask_dev, const uint32_t* type_ids_dev,
                                          int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                          float* logits_out_dev, void* stream);

/* Host-pointer variants: copy in, run, copy out, synchronise. */
KjarniErrorCode kjarni_hip_encoder_hidden_states_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                                      const uint32_t* mask, const uint32_t* type_ids,
                                                      int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                                      float* hidden_out);
KjarniErrorCode kjarni_hip_encoder_embed_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                              const uint32_t* mask, const uint32_t* type_ids,
                                              int64_t batch, int32_t seq, KjarniHipPooling pooling,
                                              int32_t normalize, KjarniHipMaskFill fill, float* out);
KjarniErrorCode kjarni_hip_encoder_logits_host(KjarniHipEncoder* enc, const uint32_t* ids,
                                               const uint32_t* mask, const uint32_t* type_ids,
                                               int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                               float* logits_out);

/* ---- several devices in one process ---------------------------------------------------
 * A group holds one replica of the model per listed device (weights replicated, ~90 MB for MiniLM).  Rows are
 * independent on this path, so a batch is cut into balanced contiguous row blocks -- floor(rows / n) each, the first
 * rows % n one more (kjarni_hip_group_shard) -- one host thread + one stream per device, no exchange inside the
 * layer loop.  This is what the string-level handles (kjarni_embedder_*, kjarni_reranker_*, kjarni_classifier_*)
 * use internally with the devices of KJARNI_HIP_DEVICES="0,1,..." (default: every visible device -- or, in a process
 * whose launcher exported LOCAL_RANK (one process per GPU), that one device; a device may be
 * listed twice); n_devices = 0 here means the same list.  A batch smaller than 8 rows per device uses fewer
 * devices, chosen in rotation. */
typedef struct KjarniHipEncoderGroup KjarniHipEncoderGroup;
KjarniErrorCode kjarni_hip_group_load(const char* model_dir, const int32_t* devices, size_t n_devices,
                                      KjarniHipEncoderGroup** out);
void kjarni_hip_group_free(KjarniHipEncoderGroup* group);
size_t kjarni_hip_group_size(const KjarniHipEncoderGroup* group);
int32_t kjarni_hip_group_device(const KjarniHipEncoderGroup* group, size_t i);
int32_t kjarni_hip_group_hidden_size(const KjarniHipEncoderGroup* group);
int32_t kjarni_hip_group_num_labels(const KjarniHipEncoderGroup* group);
/* Row block [*start_out, *start_out + *count_out) of `rows` rows that replica i owns. */
KjarniErrorCode kjarni_hip_group_shard(const KjarniHipEncoderGroup* group, int64_t rows, size_t i, int64_t* start_out,
                                       int64_t* count_out);
/* The collective that kjarni_hip_group_*_allgather issues for `rows` rows of `width` floats over n devices, as a list (host
 * arithmetic only: no device, no group needed): rank `rank` calls ncclAllGather in place (root = -1; equal blocks) or one
 * ncclBroadcast per non-empty block (root >= 0; blocks that differ by a row) on `floats` values at float offset `offset` of
 * its full output buffer.  Writes up to `cap` operations to ops_out, the total count to *count_out (n for equal blocks,
 * n x non-empty blocks otherwise). */
typedef struct KjarniHipGatherOp {
    int32_t rank;
    int32_t root;
    int64_t offset;
    int64_t floats;
} KjarniHipGatherOp;
KjarniErrorCode kjarni_hip_group_gather_plan(int64_t rows, size_t n, int64_t width, KjarniHipGatherOp* ops_out, size_t cap,
                                             size_t* count_out);
/* Host pointers: every device stages, encodes and returns its block straight into `out` ([batch, hidden] /
 * [batch, num_labels]); the mask fill follows the size of the whole call. */
KjarniErrorCode kjarni_hip_group_embed_host(KjarniHipEncoderGroup* group, const uint32_t* ids, const uint32_t* mask,
                                            const uint32_t* type_ids, int64_t batch, int32_t seq, KjarniHipPooling pooling,
                                            int32_t normalize, KjarniHipMaskFill fill, float* out);
KjarniErrorCode kjarni_hip_group_logits_host(KjarniHipEncoderGroup* group, const uint32_t* ids, const uint32_t* mask,
                                             const uint32_t* type_ids, int64_t batch, int32_t seq, KjarniHipMaskFill fill,
                                             float* logits_out);
/* Device-resident: ids_dev[i] / mask_dev[i] / type_ids_dev[i] point at replica i's row block ON device i, out_dev[i]
 * at a full [batch_total, hidden] (or [batch_total, num_labels]) buffer on device i.  Every replica computes its block
 * in place, then ONE collective leaves the whole output in every buffer: ncclAllGather over xGMI (grouped
 * ncclBroadcast when the blocks differ by a row) when the devices are distinct, peer copies otherwise.  Returns when
 * the collective has completed.  type_ids_dev may be NULL.  kjarni_hip_group_transport: "rccl" or "memcpy"
 * ("memcpy (ncclCommInitAll failed: ...)" when RCCL is present but could not build the communicator). */
KjarniErrorCode kjarni_hip_group_embed_allgather(KjarniHipEncoderGroup* group, const uint32_t* const* ids_dev,
                                                 const uint32_t* const* mask_dev, const uint32_t* const* type_ids_dev,
                                                 int64_t batch_total, int32_t seq, KjarniHipPooling pooling,
                                                 int32_t normalize, KjarniHipMaskFill fill, float* const* out_dev);
KjarniErrorCode kjarni_hip_group_logits_allgather(KjarniHipEncoderGroup* group, const uint32_t* const* ids_dev,
                                                  const uint32_t* const* mask_dev, const uint32_t* const* type_ids_dev,
                                                  int64_t batch_total, int32_t seq, KjarniHipMaskFill fill,
                                                  float* const* logits_out_dev);
const char* kjarni_hip_group_transport(KjarniHipEncoderGroup* group);

/* ---- single operators (host pointers) ---------------------------------------------
 * The kernels of the forward pass, one at a time, at the granularity of the
 * reference's own operator types: LinearLayer::matmul (+ fused epilogue),
 * EncoderSelfAttention after the QKV projection, LayerNorm::forward.  Used by the
 * single-op parity tests (tolerance 1e-5) and the kernel micro-benchmarks: when
 * iters > 0 the launch is repeated `iters` times between two HIP events and the
 * average milliseconds per launch are written to *ms_out (ms_out may be NULL). */
typedef enum KjarniHipEpilogue {
    KJARNI_HIP_EPI_BIAS = 0,
    KJARNI_HIP_EPI_BIAS_GELU = 1,
    KJARNI_HIP_EPI_BIAS_GELU_NEW = 2,
    KJARNI_HIP_EPI_BIAS_RELU = 3,
    KJARNI_HIP_EPI_BIAS_TANH = 4,
    KJARNI_HIP_EPI_BIAS_RESIDUAL = 5,
    KJARNI_HIP_EPI_BIAS_MUL_SILU = 6, /* y = silu(residual) * (x . w^T + bias): the up projection of SwiGluFeedForward over the
                                       * gate projection's output (cpu/feedforward/swiglu.rs:40-50) */
} KjarniHipEpilogue;

/* y[m,n] = epilogue(x[m,k] . w[n,k]^T + bias[n] (+ residual[m,n])); bias / residual may be NULL. */
KjarniErrorCode kjarni_hip_op_linear(int32_t device, const float* x, const float* w, const float* bias,
                                     const float* residual, int64_t m, int32_t k, int32_t n,
                                     KjarniHipEpilogue epilogue, float* y, int32_t iters, float* ms_out);
/* The same with bf16 weights (w: n x k bf16 values, row-major): the decoder's prompt projections on the bf16 matrix cores --
 * every activation split exactly into three bf16 pieces, the weights taken as they are, f32 accumulation: the products of an
 * f32 GEMM on the widened weights.  n % 128 == 0, k % 64 == 0; epilogues BIAS, BIAS_RESIDUAL, BIAS_MUL_SILU. */
KjarniErrorCode kjarni_hip_op_linear_bf16_weights(int32_t device, const float* x, const uint16_t* w_bf16, const float* bias,
                                                  const float* residual, int64_t m, int32_t k, int32_t n,
                                                  KjarniHipEpilogue epilogue, float* y, int32_t iters, float* ms_out);
/* qkv: [batch*seq, 3*heads*head_dim] (Q | K | V); mask: u32 [batch, seq] or NULL; ctx: [batch*seq, heads*head_dim]. */
KjarniErrorCode kjarni_hip_op_attention(int32_t device, const float* qkv, const uint32_t* mask, int64_t batch,
                                        int32_t seq, int32_t heads, int32_t head_dim, float mask_value,
                                        float* ctx, int32_t iters, float* ms_out);
/* The operator with the reference's full argument list (EncoderSelfAttention::forward / forward_noalloc,
 * cpu/encoder/encoder_self_attention.rs:57-140, 143-307): position_bias = NULL or an additive f32 [heads, bias_seq, bias_seq]
 * (bias_seq >= seq; broadcast over sentences; added after the 1/sqrt(head_dim) scale and before the padding mask), scale_qk = 0
 * skips the scale.  No encoder of the registry passes a bias, so models never take this entry: it runs the any-shape kernel and
 * exists so that the reference's own layer goldens (encoder_layer.rs:349-448: hidden 4, 2 heads, a position bias) run on the GPU. */
KjarniErrorCode kjarni_hip_op_attention_biased(int32_t device, const float* qkv, const uint32_t* mask, const float* position_bias,
                                               int32_t bias_seq, int64_t batch, int32_t seq, int32_t heads, int32_t head_dim,
                                               int32_t scale_qk, float mask_value, float* ctx);
/* Pooling of hidden states [batch, seq, hidden] under a u32 mask [batch, seq] (NULL = all ones), optionally followed by L2
 * normalisation: mean / cls / max / last-token pooling as kjarni-transformers/src/pooling/mod.rs:11-68 and
 * cpu/encoder/traits.rs:66-139 (l2_normalize_inplace).  out: [batch, hidden]; hidden <= 1024. */
KjarniErrorCode kjarni_hip_op_pool(int32_t device, const float* hidden_states, const uint32_t* mask, int64_t batch, int32_t seq,
                                   int32_t hidden, KjarniHipPooling pooling, int32_t normalize, float* out);
KjarniErrorCode kjarni_hip_op_layer_norm(int32_t device, const float* x, const float* gamma, const float* beta,
                                         float eps, int64_t rows, int32_t hidden, float* y, int32_t iters,
                                         float* ms_out);
/* y = LayerNorm(x . w^T + bias + residual) * gamma + beta -- the post-norm layer's residual projection with the
 * LayerNorm folded into the GEMM epilogue where the kernel covers the row width n (384, 256), otherwise GEMM + LayerNorm
 * (encoder_layer.rs:129-147, 155-176; layer_norm.rs:37-131).  bias may be NULL. */
KjarniErrorCode kjarni_hip_op_linear_layer_norm(int32_t device, const float* x, const float* w, const float* bias,
                                                const float* residual, const float* gamma, const float* beta, float eps,
                                                int64_t m, int32_t k, int32_t n, float* y, int32_t iters, float* ms_out);

/* ---- per-kernel timing (HIP events on the launch stream) -------------------------
 * profile_begin() switches the encoder into timed mode: every kernel launch of the
 * forward pass is bracketed by two hipEvents on the stream it is launched on.
 * profile_end() synchronises, resolves the events and fills up to `capacity`
 * entries (one per kernel kind of the forward pass); *count_out = entries written.
 * flops / bytes are ALGORITHMIC (2*M*N*K per GEMM, QK^T + PV for attention; every
 * operand read once and every output written once), summed over the launches. */
typedef struct KjarniHipKernelStat {
    const char* kind;   /* static string, e.g. "gemm_fc1" */
    const char* symbol; /* static string: the kernel function launched */
    uint64_t launches;
    double total_ms;
    double flops;
    double bytes;
} KjarniHipKernelStat;

KjarniErrorCode kjarni_hip_encoder_profile_begin(KjarniHipEncoder* enc);
/* Same, timing only the kernel kinds whose bit is set (bit k = k-th entry profile_end() returns):
 * fewer events on the stream when only some kernels are of interest. */
KjarniErrorCode kjarni_hip_encoder_profile_begin_kinds(KjarniHipEncoder* enc, uint32_t kinds_mask);
KjarniErrorCode kjarni_hip_encoder_profile_end(KjarniHipEncoder* enc, KjarniHipKernelStat* stats_out,
                                               size_t capacity, size_t* count_out);

/* ---- cosine scan ------------------------------------------------------------
 * corpus: f32 [n_docs, dim] row-major (the layout of vectors.bin,
 * crates/kjarni-rag/src/segment.rs:240-262).  queries: f32 [n_queries, dim].
 * mode 0 = VectorStore semantics (vector.rs:131-148: dot / max(|q||d|, 1e-9)),
 * mode 1 = Segment semantics (segment.rs:355-371: 0 when |d| < 1e-9). */
typedef enum KjarniHipCosineMode {
    KJARNI_HIP_COSINE_VECTOR_STORE = 0,
    KJARNI_HIP_COSINE_SEGMENT = 1,
} KjarniHipCosineMode;

/* scores_out_dev: f32 [n_queries, n_docs]. */
KjarniErrorCode kjarni_hip_cosine_scores(int32_t device, const float* queries_dev, int32_t n_queries,
                                         const float* corpus_dev, int64_t n_docs, int32_t dim,
                                         KjarniHipCosineMode mode, float* scores_out_dev, void* stream);

/* Top-k of a score matrix [n_queries, n_docs]: score descending, equal scores by
 * ascending document index (stable sort of an index-ordered list, vector.rs:162).
 * idx_out_dev: int64 [n_queries, k], score_out_dev: f32 [n_queries, k]; entries
 * past n_docs are (-1, -inf).  workspace_dev must hold
 * kjarni_hip_cosine_topk_workspace_bytes(n_queries, n_docs, k) bytes. */
size_t kjarni_hip_cosine_topk_workspace_bytes(int32_t n_queries, int64_t n_docs, int32_t k);
KjarniErrorCode kjarni_hip_cosine_topk(int32_t device, const float* scores_dev, int32_t n_queries,
                                       int64_t n_docs, int32_t k, void* workspace_dev,
                                       int64_t* idx_out_dev, float* score_out_dev, void* stream);

/* Scan + selection in one call on device pointers, enqueued on `stream`: per-query top-k with no caller-visible score
 * array.  One query over dim 128 / 256 / 384 / 512 / 768 / 1024 with k <= 256 runs ONE fused pass (every wave keeps its
 * best keys in registers; the scores never exist in memory) and one small merge launch.  2 .. 1 024 queries over >= 20 000
 * documents of those widths, k <= 1 024: a sample bounds every query's k-th best score, ONE bf16 pass over the corpus per
 * 64 queries keeps the documents that can reach it (the pass's rounding error is bounded and the bound relaxed by it), and
 * the survivors' cosines are taken exactly, with the f32 matrix-core scan's arithmetic; other widths (multiples of 16) from
 * 20 queries and 400 000 documents on: the f32 matrix-core scan itself selects.  Anything else runs the two calls above
 * inside the workspace.  Same order and the same scores as kjarni_hip_cosine_scores + kjarni_hip_cosine_topk, bit for bit --
 * except that with 2 .. 19 queries kjarni_hip_cosine_scores streams the corpus and sums in another order than the
 * matrix-core scan whose arithmetic the search then uses (scores within 2e-6).
 * workspace_dev: kjarni_hip_cosine_search_workspace_bytes(n_queries, n_docs, dim, k) bytes. */
size_t kjarni_hip_cosine_search_workspace_bytes(int32_t n_queries, int64_t n_docs, int32_t dim, int32_t k);
KjarniErrorCode kjarni_hip_cosine_search(int32_t device, const float* queries_dev, int32_t n_queries,
                                         const float* corpus_dev, int64_t n_docs, int32_t dim,
                                         KjarniHipCosineMode mode, int32_t k, void* workspace_dev,
                                         int64_t* idx_out_dev, float* score_out_dev, void* stream);

/* Whole search with host buffers (scan + top-k + copies + synchronise):
 * idx_out int64 [n_queries, k], score_out f32 [n_queries, k]; *n_hits_out =
 * min(k, n_docs) (0 for a Segment-mode query whose norm is < 1e-9 is reported
 * per query through idx -1). */
KjarniErrorCode kjarni_hip_cosine_search_host(int32_t device, const float* queries, int32_t n_queries,
                                              const float* corpus, int64_t n_docs, int32_t dim,
                                              KjarniHipCosineMode mode, int32_t k, int64_t* idx_out,
                                              float* score_out, int64_t* n_hits_out);

/* Where the calling thread's last kjarni_searcher_search* / kjarni_hip_index_search call spent its time, in microseconds:
 * out[0] re-opening the index, out[1] the scan over the index's device image (lookup, copies, two launches, wait), out[2] of it
 * between the query's H2D copy and the hits' arrival, out[3] the whole call; the rest is host work (BM25, rank fusion, reading
 * the hits' documents and metadata, for a Searcher the query's tokenisation and embedding).  Up to n <= 4 values. */
void kjarni_hip_search_breakdown(double* out, size_t n);

/* Keyword search (BM25, host side) walks the segments of an index of at least this many documents on a few host threads
 * (contiguous runs of segments, hits merged in segment order: the result does not depend on it).  Default 50 000; 0 = always
 * when there are four segments or more, SIZE_MAX = never.  Process-wide. */
void kjarni_hip_set_keyword_parallel_min_docs(size_t docs);

/* ---- tokenizer -----------------------------------------------------------------
 * The reference tokenises on the host with the HF `tokenizers` crate configured at
 * load time (crates/kjarni-transformers/src/pipeline/encoder/loader.rs:98-115:
 * truncation max_length = max_seq_len, padding BatchLongest, pad id 0).  This handle
 * exposes the same step (BERT WordPiece pipelines) so callers can pre-tokenise and
 * use the token-level entry points above.  Token ids are bit-exact with that crate. */
typedef struct KjarniTokenizer KjarniTokenizer;

typedef struct KjarniTokenBatch {
    uint32_t* ids;            /* [batch, seq] */
    uint32_t* attention_mask; /* [batch, seq] */
    uint32_t* type_ids;       /* [batch, seq] */
    size_t batch;
    size_t seq; /* longest sequence in the batch */
} KjarniTokenBatch;

/* max_length 0 keeps the default (512). */
KjarniErrorCode kjarni_tokenizer_load(const char* tokenizer_json_path, size_t max_length, KjarniTokenizer** out);
void kjarni_tokenizer_free(KjarniTokenizer* tok);
/* texts_b NULL: single sequences ([CLS] a [SEP]); otherwise pairs ([CLS] a [SEP] b [SEP], type ids 0/1).
 * The library allocates *out; free with kjarni_token_batch_free. */
KjarniErrorCode kjarni_tokenizer_encode_batch(const KjarniTokenizer* tok, const char* const* texts_a,
                                              const char* const* texts_b, size_t n, KjarniTokenBatch* out);
void kjarni_token_batch_free(const KjarniTokenBatch* batch);

/* ---- host-side search logic, one function at a time (parity tests) -----------------
 * BM25 tokenizer (crates/kjarni-search/src/bm25.rs:191-197), glob-match as used by
 * MetadataFilter (crates/kjarni-rag/src/index_reader.rs:54-76) and reciprocal-rank fusion
 * (crates/kjarni-search/src/hybrid.rs:3-31; ids ranked best-first, outputs hold up to
 * n_keyword + n_semantic entries). */
KjarniErrorCode kjarni_bm25_tokenize(const char* text, KjarniStringArray* out);
int32_t kjarni_glob_match(const char* pattern, const char* path);
KjarniErrorCode kjarni_rrf_fuse(const size_t* keyword_ids, size_t n_keyword, const size_t* semantic_ids,
                                size_t n_semantic, size_t limit, size_t* ids_out, float* scores_out,
                                size_t* n_out);

/* Retrieval over an on-disk index (the reference's segmented layout) with a caller-supplied query
 * embedding: Searcher::search_with_options (crates/kjarni/src/searcher/model.rs:120-187) minus the
 * encoder and the reranker.  options->mode -1 = hybrid, top_k 0 = 10; use_reranker is ignored.
 * text_query may be NULL in semantic mode, query_emb in keyword mode (which needs no GPU). */
KjarniErrorCode kjarni_hip_index_search(const char* index_path, const char* text_query, const float* query_emb,
                                        size_t dim, const KjarniSearchOptions* options, KjarniSearchResults* out);

/* ---- indexing pipeline, one host-side piece at a time (parity tests) ----------------
 * TextSplitter::split (crates/kjarni-rag/src/splitter.rs:68-120; separator NULL = "\n\n"),
 * Indexer::collect_files (crates/kjarni/src/indexer/model.rs:727-810; reads recursive, include_hidden,
 * extensions, exclude_patterns and max_file_size of the config) and IndexWriter
 * (crates/kjarni-rag/src/index_writer.rs:12-191) driven with caller-supplied embeddings:
 * texts[i], embeddings[i*dimension ..], metadata_json[i] (flat JSON object of strings, or NULL);
 * append 0 = IndexWriter::open, 1 = open_existing; max_docs_per_segment 0 = 10 000. */
KjarniErrorCode kjarni_text_split(const char* text, size_t chunk_size, size_t chunk_overlap, const char* separator,
                                  KjarniStringArray* out);
KjarniErrorCode kjarni_collect_files(const KjarniIndexerConfig* config, const char* const* inputs, size_t num_inputs,
                                     KjarniStringArray* out);
KjarniErrorCode kjarni_index_write(const char* index_path, size_t dimension, size_t max_docs_per_segment,
                                   const char* embedding_model, const char* const* texts,
                                   const char* const* metadata_json, const float* embeddings, size_t n, int32_t append);

/* ---- Whisper, one stage at a time (parity tests, benchmarks) ----------------------------
 * model_dir holds config.json (WhisperConfig, crates/kjarni-models/src/models/whisper/config.rs:11-37),
 * tokenizer.json and model.safetensors with the HF tensor names of config.rs:81-190. */
typedef struct KjarniHipWhisper KjarniHipWhisper;
KjarniErrorCode kjarni_hip_whisper_load(const char* model_dir, int32_t device, KjarniHipWhisper** out);
void kjarni_hip_whisper_free(KjarniHipWhisper* whisper);
KjarniErrorCode kjarni_hip_whisper_dims(const KjarniHipWhisper* whisper, int32_t* d_model, int32_t* n_mels, int32_t* vocab,
                                        int32_t* encoder_frames);
/* compute_mel_spectrogram, MelConfig::whisper() (crates/kjarni-transformers/src/audio/mel.rs:44-136):
 * mel_out f32 [n_mels, 3000]. */
KjarniErrorCode kjarni_hip_whisper_log_mel(KjarniHipWhisper* whisper, const float* samples, size_t num_samples, float* mel_out);
/* WhisperModel::encode_mel (whisper/transcriber.rs:122-141): mel f32 [n_mels, frames] -> hidden_out f32
 * [frames/2, d_model] (may be NULL: the result stays on the device for the decoder). */
KjarniErrorCode kjarni_hip_whisper_encode_mel(KjarniHipWhisper* whisper, const float* mel, int32_t frames, float* hidden_out);
/* log-mel + encode without leaving the device. */
KjarniErrorCode kjarni_hip_whisper_encode_audio(KjarniHipWhisper* whisper, const float* samples, size_t num_samples,
                                                float* hidden_out);
/* Decoder over the current encoder output (cpu_decoder.rs:399-516): begin = cross K/V + empty cache; forward runs
 * n <= 8 new tokens; hidden_out f32 [n, d_model] (final-normed), logits_out f32 [vocab] of the last row. */
KjarniErrorCode kjarni_hip_whisper_decode_begin(KjarniHipWhisper* whisper);
KjarniErrorCode kjarni_hip_whisper_decode_forward(KjarniHipWhisper* whisper, const uint32_t* ids, int32_t n, float* hidden_out,
                                                  float* logits_out);
/* decode_chunk's loop (transcriber.rs:144-240): generated ids, *n_out = how many (may exceed capacity). */
KjarniErrorCode kjarni_hip_whisper_greedy(KjarniHipWhisper* whisper, const uint32_t* prompt, int32_t n_prompt, int32_t timestamps,
                                          size_t max_tokens, uint32_t* ids_out, size_t capacity, size_t* n_out);
KjarniErrorCode kjarni_hip_whisper_decode_text(const KjarniHipWhisper* whisper, const uint32_t* ids, size_t n, int32_t skip_special,
                                               char** out);
/* Host-only: load_audio with the Transcriber's loader config (audio/loader.rs:125-208: mono, 16 kHz, linear
 * resampling) and the ByteLevel decode of `tokenizers` (Tokenizer::decode). */
KjarniErrorCode kjarni_audio_load_wav(const char* path, KjarniFloatArray* out, uint32_t* original_sample_rate);
KjarniErrorCode kjarni_bytelevel_decode(const char* tokenizer_json_path, const uint32_t* ids, size_t n, int32_t skip_special,
                                        char** out);

/* ---- decoder-only generation (Llama / Qwen2 / Qwen3 / Mistral layouts and GPT-2), token level --------------------
 * Qwen3 (model_type "qwen3", safetensors only; a GGUF of that architecture is refused): `head_dim` is read from config.json and
 * heads * head_dim may differ from hidden_size; every layer carries self_attn.q_norm.weight and self_attn.k_norm.weight
 * [head_dim], the per-head RMSNorm applied to Q and K before RoPE (a file without one is a load error naming it).  It runs
 * through every entry point below; the one-token step takes six launches per layer against Llama's five.
 * model_dir: config.json (crates/kjarni-models/src/models/llama/config.rs:98-158, qwen/config.rs:80-125) and
 * model.safetensors with the HF tensor names of llama/config.rs:283-330.  weights_dtype: 0 = as stored (BF16 stays
 * bf16 in HBM, other dtypes are widened to f32), 1 = f32, 2 = bf16 (f32 rounded to nearest even).  Arithmetic,
 * activations and the KV cache are f32 either way, as in the reference's bf16 LinearLayer.  max_context <= 0 =
 * max_position_embeddings.  No tokenizer is involved: prompts and results are token ids.
 * FP8 checkpoints (llama, qwen2, mistral, qwen3; single file or sharded): a linear weight `X.weight` of dtype F8_E4M3 (OCP
 * e4m3fn) beside exactly one scale tensor, `X.weight_scale_inv` or `X.weight_scale` (F32, BF16 or F16; both names mean
 * w = decode(code) * scale).  The scale's shape decides its kind: one element = per tensor, [n] or [n, 1] = per output channel,
 * [ceil(n / 128), k / 128] = 128 x 128 blocks (k % 128 == 0; n need not be a multiple of 128); every kind needs k % 16 == 0.
 * quantization_config.fmt, when present, must be "e4m3" and quantization_config.weight_block_size, when present, [128, 128];
 * input_scale tensors and activation_scheme are not read: the arithmetic is weight-only, f32 activations x dequantized weights.
 * weights_dtype 0 keeps the codes and f32 scales in HBM when the seven matrices of every layer (q/k/v/o_proj, gate/up/down_proj)
 * are all FP8 (a layer that mixes FP8 with another dtype is refused; 1 or 2 loads such a file); the embedding table and lm_head
 * stay as stored.  1 dequantizes to f32, 2 dequantizes and rounds to bf16.  A missing scale, both scale names, a scale shape that
 * fits no kind, another block size, another fmt and a NaN code (0x7F, 0xFF) in a weight are load errors that name the tensor. */
typedef struct KjarniHipDecoder KjarniHipDecoder;
KjarniErrorCode kjarni_hip_decoder_load(const char* model_dir, int32_t device, int32_t weights_dtype, int32_t max_context,
                                        KjarniHipDecoder** out);
void kjarni_hip_decoder_free(KjarniHipDecoder* decoder);
KjarniErrorCode kjarni_hip_decoder_dims(const KjarniHipDecoder* decoder, int32_t* hidden, int32_t* layers, int32_t* vocab,
                                        int32_t* context, int32_t* weights_bf16, uint64_t* weight_bytes);
KjarniErrorCode kjarni_hip_decoder_reset(KjarniHipDecoder* decoder); /* empty KV cache */
/* Prompt projections that took the 128 x 128-tile GEMM route since load (0 on NULL): a route counter for tests. */
uint64_t kjarni_hip_decoder_tile_gemm_calls(const KjarniHipDecoder* decoder);
/* kjarni_hip_decoder_generate with a repetition penalty / n-gram ban: processors on the device (default) or on a host copy
 * of the logits (0), as kjarni_hip_chat_set_device_sampling. */
void kjarni_hip_decoder_set_device_sampling(KjarniHipDecoder* decoder, int32_t on);
/* Positions held in the KV cache (0 on NULL). */
int32_t kjarni_hip_decoder_cache_len(const KjarniHipDecoder* decoder);
/* Cache rows [first, first + rows) of one layer, a read-back for tests: k_out (after RoPE; Qwen3: after the head norm and
 * RoPE) and v_out each receive f32
 * [rows, num_key_value_heads * head_dim].  An error, with nothing copied, for a layer out of range or
 * first + rows > cache_len. */
KjarniErrorCode kjarni_hip_decoder_kv_rows(const KjarniHipDecoder* decoder, int32_t layer, int32_t first, int32_t rows, float* k_out,
                                           float* v_out);
/* GGUF checkpoints (model_dir: a `.gguf` file, or a directory without safetensors that holds one; weights_dtype 0 keeps
 * Q8_0 / Q4_K / Q6_K matrices quantized in HBM, 1 dequantizes everything to f32, 2 to bf16).
 * config_json: the resolved config (config.json, or the one synthesized from GGUF metadata); free with kjarni_string_free.
 * weight_bytes_by_type: out[t] = device bytes of weights held in GGML type t (0 F32, 8 Q8_0, 12 Q4_K, 14 Q6_K, 30 BF16), t < n;
 * out[KJARNI_HIP_WEIGHT_TYPE_F8_E4M3] = the FP8 codes of an FP8 checkpoint (their scales count as F32). */
#define KJARNI_HIP_WEIGHT_TYPE_F8_E4M3 31 /* no GGML type in use here has this number */
KjarniErrorCode kjarni_hip_decoder_config_json(const KjarniHipDecoder* decoder, char** out);
KjarniErrorCode kjarni_hip_decoder_weight_bytes_by_type(const KjarniHipDecoder* decoder, uint64_t* out, size_t n);
/* Host-only GGUF views: the synthesized decoder config, and one tensor by its HF name, dequantized to f32 in HF row order
 * (*n_out = elements, may exceed capacity; shape_out[0..1] = rows, cols; *ndim_out = 1 or 2). */
KjarniErrorCode kjarni_gguf_config_json(const char* path, char** out);
KjarniErrorCode kjarni_gguf_tensor_f32(const char* path, const char* hf_name, float* out, size_t capacity, size_t* n_out, int64_t* shape_out,
                                       int32_t* ndim_out);
/* y[m, n] = x[m, k] . W^T with W given as raw GGUF blocks of type ggml_type (8 Q8_0, 12 Q4_K, 14 Q6_K; n rows of k columns) on
 * host memory, through the decoder's kernels: m < 24 in 8-row GEMV passes (Q6_K on Q8_K activation codes), m >= 24 through the
 * prompt route (dequantized weights, f32 matrix cores). */
KjarniErrorCode kjarni_hip_op_linear_ggml(int32_t device, const float* x, int64_t m, const void* blocks, int32_t ggml_type, int32_t n,
                                          int32_t k, float* y);
/* Host-only view of an FP8 checkpoint (model_dir as kjarni_hip_decoder_load; no device is needed): the F8_E4M3 matrix `hf_name`
 * read and dequantized as the loader does it, out[j, i] = decode(code) * scale in f32, with all of the loader's refusals
 * (*n_out = elements, may exceed capacity; shape_out[0..1] = rows, cols; *ndim_out = 2). */
KjarniErrorCode kjarni_fp8_tensor_f32(const char* model_dir, const char* hf_name, float* out, size_t capacity, size_t* n_out,
                                      int64_t* shape_out, int32_t* ndim_out);
/* y[m, n] = x[m, k] . W^T with W given as FP8 e4m3fn codes [n, k] and f32 scales [scale_rows, scale_cols] ([1, 1] per tensor,
 * [n, 1] per channel, [ceil(n / 128), k / 128] block) on host memory, through the decoder's FP8 kernels: m < 24 in 8-row passes
 * of the weight-streaming projection (k % 16 == 0), m >= 24 through the prompt route (weights dequantized to f32, f32 matrix
 * cores; k % 32 == 0).  A NaN code or a scale shape that fits no kind is KJARNI_ERROR_INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_linear_fp8(int32_t device, const float* x, int64_t m, const void* codes, const float* scale,
                                         int32_t scale_rows, int32_t scale_cols, int32_t n, int32_t k, float* y);
/* ---- the decode step's fused projections and their preparation kernels, alone -----------------------------------------------------
 * kjarni_hip_op_fused_proj_fp8 / _ggml: ONE call of launch_fp8_proj / launch_qfused on host arrays, every mode of the launcher
 * exposed.  mode 0 plain (1 matrix, y[0]), 1 Q | K | V (3 matrices, y[0..2]), 2 SwiGLU (gate, up; y[0]).  Arrays indexed by matrix
 * or output have 3 entries; those past the mode's count are ignored.  Matrix i is [n[i], k]: FP8 codes + f32 scales
 * [scale_rows[i], scale_cols[i]] (the kind by fp8_scale_kind; a NaN code is refused), or raw GGUF blocks of ggml_types[i] in HF row
 * order.  x [rows_alloc, ldx], of which `rows` rows and k columns are the input.  gamma [k] (may be NULL) with eps: the RMSNorm
 * prologue.  bias (may be NULL): FP8 over the concatenated columns; GGUF bias_floats floats, segment i from bias_off[i].  r
 * [rows, ldr] (may be NULL), or r_is_y0: the residual is y[0] itself, added in place.  y[i] [out_rows[i], ldy[i]] is uploaded as
 * given, written by the kernel and returned whole: y[0] rows 0 .. rows-1, y[1] / y[2] rows row_off .. row_off+rows-1.
 * offset_on_device: row_off goes to a device int that the kernel reads (row_off_ptr), and the launcher's by-value row_off gets
 * another in-range row.  GGUF Q | K | V rotates Q and K in the epilogue (head_dim, cos_t / sin_t [positions, head_dim / 2], row r at
 * position row_off + r); jobs per segment are n[i] / 2 as the decoder derives them.  q8k: the rows go through launch_qprep first
 * (RMSNorm when gamma, Q8_K codes), as the decoder does for Q6_K linears; xn_out [rows, k] (written when gamma), xq_out [rows, k]
 * and xd_out [rows, k / 256] (each may be NULL) then return what the device produced.
 * INVALID_CONFIG, before any GPU work and with the outputs untouched: rows that do not fit out_rows, positions past the table, ldx /
 * ldy / ldr that do not cover their columns, ldx % 4, gate and up of different n, Q / K rows no multiple of head_dim, bias_off
 * outside bias_floats; and, after the upload, whatever the launcher itself refuses (rows outside 1 .. 8, k % 16 / k % 256, ...). */
KjarniErrorCode kjarni_hip_op_fused_proj_fp8(int32_t device, int32_t mode, const void* const* codes, const float* const* scales,
                                             const int32_t* scale_rows, const int32_t* scale_cols, const int32_t* n, int32_t k,
                                             const float* x, int32_t rows_alloc, int64_t ldx, int32_t rows, const float* gamma, float eps,
                                             const float* bias, const float* r, int64_t ldr, int32_t r_is_y0, float* const* y,
                                             const int32_t* out_rows, const int64_t* ldy, int32_t row_off, int32_t offset_on_device);
KjarniErrorCode kjarni_hip_op_fused_proj_ggml(int32_t device, int32_t mode, const void* const* blocks, const int32_t* ggml_types,
                                              const int32_t* n, int32_t k, const float* x, int32_t rows_alloc, int64_t ldx, int32_t rows,
                                              const float* gamma, float eps, const float* bias, int32_t bias_floats, const int32_t* bias_off,
                                              const float* r, int64_t ldr, int32_t r_is_y0, float* const* y, const int32_t* out_rows,
                                              const int64_t* ldy, int32_t row_off, int32_t offset_on_device, int32_t head_dim,
                                              const float* cos_t, const float* sin_t, int32_t positions, int32_t q8k, float* xn_out,
                                              int8_t* xq_out, float* xd_out);
/* launch_qembed alone: out [n_ids, k] (uploaded as given, returned whole) = the dequantized rows ids[i] of the table [vocab, k]
 * given as raw GGUF blocks; an id >= vocab gives zeros. */
KjarniErrorCode kjarni_hip_op_qembed(int32_t device, const uint32_t* ids, int32_t n_ids, const void* blocks, int32_t ggml_type, int32_t vocab,
                                     int32_t k, float* out);
/* launch_q8k_quantize alone: x [rows, ldx] -> codes_out [rows, k] (int8), scales_out [rows, k / 256], deq_out [rows, k]. */
KjarniErrorCode kjarni_hip_op_q8k_quantize(int32_t device, const float* x, int32_t rows, int64_t ldx, int32_t k, int8_t* codes_out,
                                           float* scales_out, float* deq_out);
/* CpuDecoder::forward + final norm + lm head (llama/cpu_decoder.rs:196-219): appends n tokens to the cache.  Fewer
 * than 24 tokens run 8 rows at a time; longer prompts (when the geometry allows) go through the matrix-core route in
 * 2 048-row chunks.  hidden_out receives the final-normed rows of the LAST 8-row block, f32 [((n-1) mod 8) + 1, hidden];
 * logits_out f32 [vocab] of the last position.  Either may be NULL. */
KjarniErrorCode kjarni_hip_decoder_forward(KjarniHipDecoder* decoder, const uint32_t* ids, int32_t n, float* hidden_out,
                                           float* logits_out);
/* run_generation_loop with DecodingStrategy::Greedy (crates/kjarni-transformers/src/decoder/generator.rs:228-381):
 * prefill, then up to max_new_tokens tokens; stops at an eos id of config.json (not emitted) or the context limit.
 * repetition_penalty 1.0 and no_repeat_ngram_size 0 switch those processors off (common/sampling.rs:207-235).
 * on_token (may be NULL; text is NULL here) returning false stops.  *n_out = tokens generated (may exceed capacity). */
KjarniErrorCode kjarni_hip_decoder_generate(KjarniHipDecoder* decoder, const uint32_t* prompt, size_t n_prompt, size_t max_new_tokens,
                                            float repetition_penalty, int32_t no_repeat_ngram_size, KjarniTokenCallbackFn on_token,
                                            void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out);

/* ---- lanes: up to 8 prompts decoded in lock step (NOT in the reference: it generates one sequence at a time) ----
 * A lane is one sequence with its own KV cache and position; at most 8 lanes run per step, a call may carry any number of
 * prompts, and a lane that finishes takes the next waiting prompt.
 *
 * kjarni_hip_decoder_generate_batch: prompt i is prompt_ids[offsets[i] .. offsets[i + 1]) (n + 1 offsets) and generates up to
 * max_new_tokens[i] tokens under the rules of kjarni_hip_decoder_generate (stop token not emitted, context limit); the ids
 * are the ones that call gives for the prompt alone.  lanes: 1..8, 0 = 8.  lane_context: rows of each lane's cache,
 * <= 0 = the decoder's context (a lane stops where its cache is full).  on_token (may be NULL) gets the prompt's index and is
 * called in step order, lane order within a step; false ends that prompt only.  Prompt i's ids go to
 * ids_out[i * capacity ..], n_out[i] = tokens generated (may exceed capacity).  n == 0: OK, nothing written.  lanes outside
 * 0..8, or a prompt longer than a lane (the message names its index): INVALID_CONFIG before any GPU work. */
typedef bool (*KjarniBatchTokenCallbackFn)(size_t prompt_index, KjarniToken token, void* user_data);
KjarniErrorCode kjarni_hip_decoder_generate_batch(KjarniHipDecoder* decoder, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                  const size_t* max_new_tokens, float repetition_penalty, int32_t no_repeat_ngram_size,
                                                  int32_t lanes, int32_t lane_context, KjarniBatchTokenCallbackFn on_token, void* user_data,
                                                  uint32_t* ids_out, size_t capacity, size_t* n_out);
/* Test hooks (as kjarni_hip_decoder_forward / _kv_rows): empty lane caches for `lanes` lanes; a prompt into one lane; one
 * lock-step step over ids[lanes] for the lanes with live[lane] != 0 (NULL: all; a frozen lane's cache is neither read nor
 * written, its output rows are unspecified) -> final-normed hidden rows [lanes, hidden] and logits [lanes, vocab] (either
 * may be NULL); a lane's cache length (-1: no such lane) and rows; the lanes' capacity; how many projections of lane steps
 * took the multi-row weight-streaming kernel / fell back to the one-wave-per-column kernel since load. */
KjarniErrorCode kjarni_hip_decoder_lanes_begin(KjarniHipDecoder* decoder, int32_t lanes, int32_t lane_context);
KjarniErrorCode kjarni_hip_decoder_lane_prefill(KjarniHipDecoder* decoder, int32_t lane, const uint32_t* ids, int32_t n);
KjarniErrorCode kjarni_hip_decoder_lanes_step(KjarniHipDecoder* decoder, const uint32_t* ids, const int32_t* live, float* hidden_out,
                                              float* logits_out);
int32_t kjarni_hip_decoder_lane_cache_len(const KjarniHipDecoder* decoder, int32_t lane);
int32_t kjarni_hip_decoder_lane_capacity(const KjarniHipDecoder* decoder);
KjarniErrorCode kjarni_hip_decoder_lane_kv_rows(const KjarniHipDecoder* decoder, int32_t lane, int32_t layer, int32_t first, int32_t rows,
                                                float* k_out, float* v_out);
void kjarni_hip_decoder_lane_gemv_calls(const KjarniHipDecoder* decoder, uint64_t* streamed, uint64_t* fallback);
/* The lane count kjarni_generator_generate_batch runs with (1..8, 0 = 8, the default). */
KjarniErrorCode kjarni_hip_generator_set_lanes(KjarniGenerator* generator, int32_t lanes);

/* ---- wide lanes: up to 64 prompts decoded in lock step on the matrix cores (NOT in the reference) ----
 * kjarni_hip_decoder_generate_wide is kjarni_hip_decoder_generate_batch with lanes 1..64 (0 = 64).  An effective width
 * min(lanes, n) of 8 or less runs generate_batch's own step; 9..64 runs every projection of the step as one 64-row tile of the
 * prompt GEMM (the weights are read once per step whatever the width), the rest being the lanes' kernels.  Results, callback
 * order, stop rules and lane turnover are generate_batch's.  The lane caches take 2 * layers * lanes * rows * kv_heads *
 * head_dim * 4 bytes with rows = min(context, lane_context) -- 64 KB per token per lane on the Llama-1B shape -- so set
 * lane_context.  INVALID_CONFIG before any GPU work: lanes outside 0..64, an empty prompt or one longer than a lane (the
 * message names its index), more than 16 stop ids, and above 8 lanes a quantized (GGUF) or FP8 checkpoint (the prompt GEMM would
 * dequantize every matrix in every step) or widths that are no multiples of 32. */
KjarniErrorCode kjarni_hip_decoder_generate_wide(KjarniHipDecoder* decoder, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                 const size_t* max_new_tokens, float repetition_penalty, int32_t no_repeat_ngram_size,
                                                 int32_t lanes, int32_t lane_context, KjarniBatchTokenCallbackFn on_token, void* user_data,
                                                 uint32_t* ids_out, size_t capacity, size_t* n_out);
/* Test hooks of the wide route, as the lane hooks above.  wide_begin takes 9..64 lanes (0 = 64): 8 or fewer are refused, that
 * width is kjarni_hip_decoder_lanes_begin's. */
KjarniErrorCode kjarni_hip_decoder_wide_begin(KjarniHipDecoder* decoder, int32_t lanes, int32_t lane_context);
KjarniErrorCode kjarni_hip_decoder_wide_prefill(KjarniHipDecoder* decoder, int32_t lane, const uint32_t* ids, int32_t n);
KjarniErrorCode kjarni_hip_decoder_wide_prefill_shared(KjarniHipDecoder* decoder, int32_t lane, int32_t shared, const uint32_t* ids,
                                                       int32_t n);
KjarniErrorCode kjarni_hip_decoder_wide_step(KjarniHipDecoder* decoder, const uint32_t* ids, const int32_t* live, float* hidden_out,
                                             float* logits_out);
int32_t kjarni_hip_decoder_wide_cache_len(const KjarniHipDecoder* decoder, int32_t lane);
int32_t kjarni_hip_decoder_wide_capacity(const KjarniHipDecoder* decoder);
KjarniErrorCode kjarni_hip_decoder_wide_kv_rows(const KjarniHipDecoder* decoder, int32_t lane, int32_t layer, int32_t first, int32_t rows,
                                                float* k_out, float* v_out);
/* 1..64: kjarni_generator_generate_batch runs generate_wide with that width; 0 (the default) = off, the lanes path as set by
 * kjarni_hip_generator_set_lanes. */
KjarniErrorCode kjarni_hip_generator_set_wide_lanes(KjarniGenerator* generator, int32_t lanes);

/* ---- prompt-lookup speculative decoding (NOT in the reference) ----
 * Greedy generation that emits several tokens per step.  T = the prompt and every token so far; a step drafts the
 * continuation of a match of T's suffix inside T: over every position e (a continuation would start at T[e]) whose
 * preceding ngram_min..ngram_max tokens equal T's last ones, the longest match, then the longest continuation (up to
 * draft_tokens), then the latest.  The last token and the draft run as ONE causal block of draft_tokens + 1 rows, every row
 * through the vocabulary head; the model's own argmax tokens are kept up to and including the first that differs from the
 * draft, so every emitted token is an argmax of the model's logits: the ids are kjarni_hip_decoder_generate's whenever the
 * two best logits are further apart than the float bar at every step (the multi-row kernels sum in another order).  Off
 * unless asked for; sampling, repetition penalty and the n-gram ban keep their own paths. */
typedef struct KjarniHipLookupConfig { int32_t draft_tokens, ngram_max, ngram_min; } KjarniHipLookupConfig;  /* 1..7, 1..4, 1..ngram_max */
typedef struct KjarniHipLookupStats { uint64_t verify_steps, drafted_tokens, accepted_tokens, single_row_steps; } KjarniHipLookupStats;
KjarniHipLookupConfig kjarni_hip_lookup_config_default(void);   /* 7, 3, 1 */
/* kjarni_hip_decoder_generate with repetition_penalty 1 and no n-gram ban, through the lookup loop.  stop_ids / n_stop: the
 * ids that end the call (not emitted); n_stop == 0: config.json's eos ids.  config NULL: the default.  stats (may be NULL)
 * covers the steps whose tokens the host consumed: verify_steps (two or more rows), single_row_steps (one row: the last
 * free row of the cache), drafted_tokens and accepted_tokens summed over both.  A config outside the ranges or a prompt longer
 * than the context: INVALID_CONFIG before any GPU work, the message names the field. */
KjarniErrorCode kjarni_hip_decoder_generate_lookup(KjarniHipDecoder* decoder, const uint32_t* prompt, size_t n_prompt, size_t max_new_tokens,
                                                   const uint32_t* stop_ids, size_t n_stop, const KjarniHipLookupConfig* config,
                                                   KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out, size_t capacity,
                                                   size_t* n_out, KjarniHipLookupStats* stats);
/* The draft kernel alone on a host-given history: draft_out[7], *n_out = draft length. */
KjarniErrorCode kjarni_hip_op_lookup_draft(int32_t device, const uint32_t* tokens, size_t n, const KjarniHipLookupConfig* config,
                                           uint32_t* draft_out, int32_t* n_out);
/* The token-selection kernels alone, on logits given by the host; each entry runs the launcher the models run, on scratch
 * zero-initialised as theirs, with a guard band behind every output buffer (INFERENCE_FAILED when one is touched, or when
 * the kernels leave device state other than the contract of their launcher).
 *
 * kjarni_hip_op_argmax: `calls` independent greedy picks over logits [calls, rows, ld] (ld >= vocab), the last of equal
 * maxima wins.  DECODER: rows == 1, the replayed single-sequence pick.  LANES: rows <= 8, live[rows] says which lanes pick;
 * picks_out of a frozen lane is -1 and its token / history must come back untouched.  LOOKUP: rows <= 8, the verify pick with
 * the draft draft[calls, n_draft] (n_draft <= rows - 1): accepted_out[call] = a, the longest prefix of the draft that equals
 * the rows' own picks; picks_out[call, 0..a] = p_0..p_a, -1 past them.  picks_out is [calls, rows]. */
typedef enum KjarniHipArgmaxRoute { KJARNI_HIP_ARGMAX_DECODER = 0, KJARNI_HIP_ARGMAX_LANES = 1, KJARNI_HIP_ARGMAX_LOOKUP = 2 } KjarniHipArgmaxRoute;
KjarniErrorCode kjarni_hip_op_argmax(int32_t device, const float* logits, int32_t calls, int32_t rows, int64_t ld, int32_t vocab, int32_t route,
                                     const int32_t* live, const uint32_t* draft, int32_t n_draft, int32_t* picks_out, int32_t* accepted_out);
/* Whisper's pick (argmax over the ids that may be produced, the last of equal maxima wins; eos when none can) over logits
 * [calls, lanes, vocab], lanes <= 8: two_launch == 0 the one-workgroup-per-lane kernel, else the two-launch form of the replayed
 * step.  tokens_out is [calls, lanes]. */
KjarniErrorCode kjarni_hip_op_whisper_pick(int32_t device, const float* logits, int32_t calls, int32_t lanes, int32_t vocab,
                                           int32_t first_special, int32_t eos, int32_t timestamp_begin, int32_t allow_timestamps,
                                           int32_t two_launch, int32_t* tokens_out);
/* Repetition penalty and n-gram ban (0 = off) of the history tokens[n] on logits[vocab], the per-token counts built as a
 * generate call builds them: one launch over the first n_bulk tokens, one per later token.  Ids >= vocab are ignored. */
KjarniErrorCode kjarni_hip_op_logits_processors(int32_t device, const float* logits, int32_t vocab, const uint32_t* tokens, int32_t n,
                                                int32_t n_bulk, float repetition_penalty, int32_t no_repeat_ngram, float* logits_out);
/* The sampler's cut: what the device hands to the host per sampled token.  Row c of `logits` holds vocabs[c] floats, the rows
 * packed one after another; the calls run in order on ONE scratch, header and candidate buffer, as consecutive tokens of a
 * generate call do.  top_k / top_p / min_p negative = not set.  Per call: the header, and in ids_out / logits_out
 * [calls, capacity] the first min(count, capacity) candidates (every token with logit >= floor, in no particular order).
 * overflow = 1: count exceeds the capacity, or no cut could be placed -- the list is not usable. */
typedef struct KjarniHipSampleHeader { float mx, sum, floor; uint32_t count, overflow; } KjarniHipSampleHeader;
KjarniErrorCode kjarni_hip_op_sample_candidates(int32_t device, const float* logits, const int32_t* vocabs, int32_t calls, int64_t top_k,
                                                float top_p, float min_p, int32_t capacity, KjarniHipSampleHeader* headers_out,
                                                uint32_t* ids_out, float* logits_out);
/* Host restatement of the same rule (no GPU). */
KjarniErrorCode kjarni_lookup_draft(const uint32_t* tokens, size_t n, const KjarniHipLookupConfig* config, uint32_t* draft_out,
                                    int32_t* n_out);
/* Test hook: one verify step with an explicit draft on the cache as it stands (after kjarni_hip_decoder_forward): `rows` in
 * n_draft + 1 .. 8 rows are computed (the rows past the draft repeat its last id); tokens_out[0 .. *n_accepted] (room for 8) are
 * the picks, the cache grows by *n_accepted + 1; logits_out (may be NULL) f32 [n_draft + 1, vocab], every row: row i is the
 * model's output after token, draft[0..i).  n_draft outside 0..7, rows outside n_draft + 1 .. 8 or cache_len + rows > context:
 * INVALID_CONFIG before any GPU work. */
KjarniErrorCode kjarni_hip_decoder_verify_step(KjarniHipDecoder* decoder, uint32_t token, const uint32_t* draft, int32_t n_draft,
                                               int32_t rows, uint32_t* tokens_out, int32_t* n_accepted, float* logits_out);
/* ---- prompt-lookup decoding for sampled requests (NOT in the reference) ----
 * Lookup drafts are deterministic, so no rejection scheme is needed: the plain loop decides token i as a function of (processed
 * logits, the i-th draw); a verify step decides row 0 with the next draw and, while the result equals the draft, the next row
 * with the draw after it; the first token that differs is kept.  Draws are taken one per decided row, never for a row that is
 * not reached: the ids are the plain loop's for the same draw stream.  The n-gram ban is not built for rows. */
typedef struct KjarniHipSamplingOptions {
    size_t max_new_tokens;
    float repetition_penalty;     /* 1 = off */
    int32_t no_repeat_ngram;      /* 0 = off */
    int32_t sample;               /* 0 = greedy */
    float temperature;
    int64_t top_k;                /* < 0 = not set */
    float top_p, min_p;           /* < 0 = not set */
    const uint32_t* stop_ids;     /* n_stop == 0: config.json's eos ids */
    size_t n_stop;
    const float* uniforms;        /* token i uses uniforms[i]; NULL: a generator seeded with `seed` */
    size_t n_uniforms;            /* >= max_new_tokens when uniforms is given, else INVALID_CONFIG before any GPU work */
    uint64_t seed;
} KjarniHipSamplingOptions;
/* sizeof(KjarniHipSamplingOptions) and the offset of every field in declaration order, as this library was compiled (a binding
 * checks its mirror against it): writes min(14, capacity) values, returns 14. */
size_t kjarni_hip_sampling_options_layout(size_t* out, size_t capacity);
/* kjarni_hip_decoder_generate with these options.  lookup NULL: the plain loop (the token-level API with sampling).  lookup
 * given: the sampled lookup loop when options->sample and no n-gram ban; greedy without processors takes
 * kjarni_hip_decoder_generate_lookup's loop; greedy with a penalty, or any n-gram ban, the plain loop (stats zero).  stats as
 * kjarni_hip_decoder_generate_lookup.  A lookup config outside its ranges, a prompt longer than the context or an empty
 * prompt: INVALID_CONFIG before any GPU work. */
KjarniErrorCode kjarni_hip_decoder_generate_sampled(KjarniHipDecoder* decoder, const uint32_t* prompt, size_t n_prompt,
                                                    const KjarniHipSamplingOptions* options, const KjarniHipLookupConfig* lookup,
                                                    KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out, size_t capacity,
                                                    size_t* n_out, KjarniHipLookupStats* stats);
/* Tokens of sampled / processed requests decided from the device's candidates, and those that needed a logits row, since load. */
void kjarni_hip_decoder_sampling_routes(const KjarniHipDecoder* decoder, uint64_t* from_candidates, uint64_t* from_logits);
/* Test hook: kjarni_hip_decoder_verify_step for a sampled request (options->sample != 0, no n-gram ban).  history[n_history]:
 * the tokens the repetition penalty counts, the last of them `token` (not read when the penalty is 1).  uniforms[n_draft + 1]:
 * one draw per decided row.  picks_out[0 .. *accepted_out] (room for 8), *draws_used_out = *accepted_out + 1; logits_out (may
 * be NULL) f32 [n_draft + 1, vocab]: the processed rows.  The cache grows by *accepted_out + 1.  Ranges as
 * kjarni_hip_decoder_verify_step: INVALID_CONFIG before any GPU work. */
KjarniErrorCode kjarni_hip_decoder_verify_step_sampled(KjarniHipDecoder* decoder, uint32_t token, const uint32_t* draft, int32_t n_draft,
                                                       int32_t rows, const KjarniHipSamplingOptions* options, const uint32_t* history,
                                                       size_t n_history, const float* uniforms, uint32_t* picks_out,
                                                       int32_t* accepted_out, int32_t* draws_used_out, float* logits_out);
/* The sampler's cut over `rows` (1..8) logits rows of stride ld >= vocab in one chain of three launches.  Per row r: headers_out[r]
 * and, in ids_out / logits_out [rows, capacity], its first min(count, capacity) candidates.  A guard band lies behind every
 * row's `capacity` slots, behind the headers and behind every row's scratch (INFERENCE_FAILED when one is touched). */
KjarniErrorCode kjarni_hip_op_sample_candidates_rows(int32_t device, const float* logits, int64_t ld, int32_t rows, int32_t vocab,
                                                     int64_t top_k, float top_p, float min_p, int32_t capacity,
                                                     KjarniHipSampleHeader* headers_out, uint32_t* ids_out, float* logits_out);
/* The repetition penalty over the rows of a verify block: logits [rows, ld]; history[n_history] ends with ids[0]; row r is
 * penalised for the history plus ids[1..r], once per occurrence.  logits_out [rows, ld] (the padding comes back untouched). */
KjarniErrorCode kjarni_hip_op_repetition_penalty_rows(int32_t device, const float* logits, int64_t ld, int32_t rows, int32_t vocab,
                                                      const uint32_t* ids, const uint32_t* history, int32_t n_history, float penalty,
                                                      float* logits_out);
/* Deciding a block on the host (the specification of the device path): logits [rows, ld] already processed, draft[n_draft];
 * row by row the distribution of kjarni_sampling_distribution and kjarni_sample_from_probs with uniforms[r]; stops after the
 * first pick that differs from the draft or after row min(n_draft, rows - 1).  picks_out[0 .. *accepted_out],
 * *draws_used_out = *accepted_out + 1; draft entries from the first rejection on are not read. */
KjarniErrorCode kjarni_lookup_accept_sampled(const float* logits, int64_t ld, int32_t rows, size_t vocab, const uint32_t* draft,
                                             int32_t n_draft, float temperature, int64_t top_k, float top_p, float min_p,
                                             const float* uniforms, uint32_t* picks_out, int32_t* accepted_out, int32_t* draws_used_out);
/* Projections of verify steps that took the multi-row weight-streaming kernel / fell back to the one-wave-per-column kernel
 * since load (counted when enqueued: a replayed graph counts once, at capture). */
void kjarni_hip_decoder_verify_gemv_calls(const KjarniHipDecoder* decoder, uint64_t* streamed, uint64_t* fallback);
/* Prompt lookup for kjarni_generator_generate / _generate_stream: 0 = off (the default), 1..7 drafted tokens per step.  Used
 * when the resolved config is greedy with repetition_penalty 1 and no n-gram ban; generate_batch and Chat are untouched. */
KjarniErrorCode kjarni_hip_generator_set_prompt_lookup(KjarniGenerator* generator, int32_t draft_tokens);
/* kjarni_hip_decoder_verify_gemv_calls of the generator's model: it moves only when a call took the lookup loop. */
void kjarni_hip_generator_verify_gemv_calls(KjarniGenerator* generator, uint64_t* streamed, uint64_t* fallback);
/* Prompt lookup for sampled configs (with or without a repetition penalty): off by default.  When on, prompt lookup is set
 * (1..7) and the resolved config has no n-gram ban, generate / generate_stream / send take the sampled lookup loop; the draws
 * come from the handle's generator exactly as on the plain path.  Otherwise nothing changes. */
KjarniErrorCode kjarni_hip_generator_set_prompt_lookup_sampling(KjarniGenerator* generator, int32_t on);
KjarniErrorCode kjarni_hip_chat_set_prompt_lookup_sampling(KjarniChat* chat, int32_t on);

/* ---- speculative decoding with a draft model (NOT in the reference) ----
 * The verify step of prompt lookup with the draft coming from `draft`, a second decoder on the same device with the same vocab
 * and a context at least the decoder's.  Per round the drafter proposes draft_tokens tokens greedily (one 2-row pass that
 * re-runs the last cached row, then one-row steps), the decoder verifies them in one multi-row step, and every emitted token
 * is the decoder's own decision: the ids are those of kjarni_hip_decoder_generate_sampled without lookup for the same options
 * and draws (greedy: wherever the two best logits are further apart than the float bar).  A round is one captured chain on the
 * decoder's stream.  draft_tokens (1..7) is required: DESIGN §6 has the table a caller chooses from.  Routing: greedy without
 * processors -> the greedy loop; options->sample without an n-gram ban (with or without a repetition penalty) -> the sampled
 * loop; greedy with a penalty, or any n-gram ban -> the plain loop (stats zero, the drafter untouched).  stats as
 * kjarni_hip_decoder_generate_lookup: drafted_tokens = rows - 1 per verify step.  draft NULL, draft == decoder, another
 * device, another vocab, a shorter context, draft_tokens outside 1..7, an empty or over-long prompt: INVALID_CONFIG before any
 * GPU work, the message names the argument.  Afterwards the drafter's cache is one row behind the decoder's. */
KjarniErrorCode kjarni_hip_decoder_generate_draft(KjarniHipDecoder* decoder, KjarniHipDecoder* draft, const uint32_t* prompt, size_t n_prompt,
                                                  const KjarniHipSamplingOptions* options, int32_t draft_tokens,
                                                  KjarniTokenCallbackFn on_token, void* user_data, uint32_t* ids_out, size_t capacity,
                                                  size_t* n_out, KjarniHipLookupStats* stats);
/* Test hook: one greedy round of `rows` (2..8) rows on the two caches as they stand, like kjarni_hip_decoder_verify_step with
 * the draft coming from the drafter.  `token` is the token in neither cache; the one before it is the last of the decoder's
 * resident tokens, which must cover its cache (>= 1 row); the drafter's resident tokens must be the decoder's up to
 * cache_len - 1, else INVALID_CONFIG.  draft_out[rows - 1] (room for 7): the proposals; tokens_out[0 .. *n_accepted] (room for
 * 8): the picks; logits_out (may be NULL) f32 [rows, vocab].  The decoder's cache grows by *n_accepted + 1; the drafter's ends
 * at the decoder's length, or one row short when every proposal was accepted. */
KjarniErrorCode kjarni_hip_decoder_draft_round(KjarniHipDecoder* decoder, KjarniHipDecoder* draft, uint32_t token, int32_t rows,
                                               uint32_t* draft_out, uint32_t* tokens_out, int32_t* n_accepted, float* logits_out);
/* A drafter for kjarni_generator_generate / _generate_stream and kjarni_chat_send*: loads model_dir_or_gguf on the handle's
 * device with its weights as stored and the handle's context; the handle owns it.  NULL or draft_tokens == 0 frees it.  While
 * set it takes precedence over prompt lookup, under the routing of kjarni_hip_decoder_generate_draft; generate_batch is
 * untouched.  draft_tokens outside 0..7 or a checkpoint with another vocab: INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_generator_set_draft_model(KjarniGenerator* generator, const char* model_dir_or_gguf, int32_t draft_tokens);
KjarniErrorCode kjarni_hip_chat_set_draft_model(KjarniChat* chat, const char* model_dir_or_gguf, int32_t draft_tokens);
/* kjarni_hip_decoder_verify_gemv_calls of the chat's model: it moves only when a call took a lookup or a draft loop. */
void kjarni_hip_chat_verify_gemv_calls(KjarniChat* chat, uint64_t* streamed, uint64_t* fallback);

/* ---- scoring: per-token log-probabilities of a given sequence (NOT in the reference: it has no scoring entry point; the
 * arithmetic is its final norm + head, llama/cpu_decoder.rs:196-219, gpt2/cpu_decoder.rs:371-394, and log_softmax_1d,
 * common/sampling.rs:200-205) ----
 * kjarni_hip_decoder_score resets the cache and runs ids[0, n) through the routes of kjarni_hip_decoder_forward.  For every
 * position p in [first, n), 1 <= first < n, entry p - first of the outputs (n - first entries each, any may be NULL) is
 * log p(ids[p] | ids[0, p)), the arg-max token of that distribution (the last of equal maxima) and the arg-max's
 * log-probability.  Only the rows first - 1 .. n - 2 reach the vocabulary head.  The fused route (f32 / bf16 heads, hidden a
 * multiple of 32) runs the head on the fp32 matrix cores and never stores the logits; the rows route (quantized heads, other
 * geometries, or set_score_fused(0)) takes 8 materialised logits rows at a time.  Afterwards the decoder is in the state
 * reset + forward(ids, n) leaves.  n < 2, first outside [1, n), n > context or an id >= vocab: INVALID_CONFIG before any GPU
 * work, the message names the argument. */
KjarniErrorCode kjarni_hip_decoder_score(KjarniHipDecoder* decoder, const uint32_t* ids, int32_t n, int32_t first, float* logprob_out,
                                         uint32_t* top_out, float* top_logprob_out);
void kjarni_hip_decoder_set_score_fused(KjarniHipDecoder* decoder, int32_t on);   /* default on; 0: every checkpoint takes the rows route */
/* Head launches of kjarni_hip_decoder_score by route since load (zeros on NULL). */
void kjarni_hip_decoder_score_calls(const KjarniHipDecoder* decoder, uint64_t* fused, uint64_t* rows);
/* The head kernels alone, host pointers (as kjarni_hip_op_linear_ggml): hidden f32 [m, k]; W [vocab, k] f32 (bf16 = 0) or
 * bf16 bits (bf16 = 1); targets [m]; slab_tiles 0 = automatic; fused 0 = the rows route (materialised in 8-row blocks).
 * Outputs [m] each, any may be NULL: log-probability of the target, arg-max, its log-probability, the row's log-sum-exp. */
KjarniErrorCode kjarni_hip_op_score_head(int32_t device, const float* hidden, int64_t m, int32_t k, const void* W, int32_t bf16,
                                         int32_t vocab, const uint32_t* targets, int32_t slab_tiles, int32_t fused, float* logprob_out,
                                         uint32_t* top_out, float* top_logprob_out, float* lse_out);

/* Top-k alternatives per scored position.  kjarni_hip_decoder_score_topk is kjarni_hip_decoder_score with, instead of the arg-max
 * alone, the top_k most likely tokens of every position: topk_ids_out / topk_logprob_out are [n - first, top_k] row-major, slot j
 * the token with the j-th largest logit (equal logits: the larger id first) and its log-probability, non-increasing along a row;
 * slot 0 is kjarni_hip_decoder_score's top / top_logprob and logprob_out is its logprob_out, bit for bit.  The fused route keeps a
 * sorted list of KJARNI_SCORE_TOPK_MAX candidates per lane next to the running sums (the logits are still never stored); the rows
 * route takes them from the materialised rows.  Same routes, chunks, prefix reuse, counters and final state as
 * kjarni_hip_decoder_score, and its argument errors; top_k outside [1, KJARNI_SCORE_TOPK_MAX] or above the vocabulary:
 * INVALID_CONFIG naming top_k before any GPU work, the cache untouched.  Any output may be NULL. */
#ifndef KJARNI_SCORE_TOPK_MAX
#define KJARNI_SCORE_TOPK_MAX 8
#endif
KjarniErrorCode kjarni_hip_decoder_score_topk(KjarniHipDecoder* decoder, const uint32_t* ids, int32_t n, int32_t first, int32_t top_k,
                                              float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out);
/* kjarni_hip_op_score_head with top_k: topk_ids_out / topk_logprob_out [m, top_k], logprob_out / lse_out [m], any may be NULL.
 * logprob, lse and slot 0 are bit-identical to kjarni_hip_op_score_head's with the same slab_tiles and route. */
KjarniErrorCode kjarni_hip_op_score_head_topk(int32_t device, const float* hidden, int64_t m, int32_t k, const void* W, int32_t bf16,
                                              int32_t vocab, const uint32_t* targets, int32_t slab_tiles, int32_t fused, int32_t top_k,
                                              float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out, float* lse_out);

/* ---- prefix reuse: keep the cached rows of the tokens a call shares with what the cache holds (NOT in the reference, whose
 * generator clears its cache per call, generator.rs:228-260) ----
 * Off by default.  On: kjarni_hip_decoder_generate / _generate_lookup / _generate_sampled keep the cache rows of
 * kjarni_hip_prefix_keep(resident tokens, prompt, n_prompt - 1) and forward the rest of the prompt; kjarni_hip_decoder_score
 * keeps at most first - 1 rows; kjarni_hip_decoder_generate_batch prefills the prefix all its prompts share (one token short of
 * the shortest prompt) once, into the single-sequence cache, and copies its rows into every lane that takes a request.  Kept
 * rows were computed by whichever route wrote them (a reply's rows by one-row decode steps, where a full prefill runs the
 * prompt GEMM), so logits and cache rows are the reuse-off values inside the decoder's float bar and the ids are the same
 * wherever the two best logits are further apart than that.  A NULL handle is ignored. */
void kjarni_hip_decoder_set_prefix_reuse(KjarniHipDecoder* decoder, int32_t on);
/* FP8 checkpoints on the matrix cores (off by default; a no-op on a checkpoint that is not FP8; a NULL handle is ignored).  On:
 * the prompt projections of up to a few hundred rows multiply the FP8 codes themselves on the bf16 matrix cores
 * (launch_prefill_gemm_fp8) instead of writing every matrix as f32 first, and the checkpoint is accepted on the wide lanes
 * (9 .. 64), whose step then runs Q, K, V and the MLP through the same GEMM.  Off: everything enqueued is what it was before the
 * switch existed, the refusal above 8 lanes included.  Flipping it drops the captured wide-step graphs.
 * kjarni_hip_decoder_fp8_matrix_cores reads it back (0 for NULL). */
void kjarni_hip_decoder_set_fp8_matrix_cores(KjarniHipDecoder* decoder, int32_t on);
int32_t kjarni_hip_decoder_fp8_matrix_cores(const KjarniHipDecoder* decoder);
/* Prompt tokens whose rows were kept / computed by the calls that ran with reuse on, since load (zeros on NULL; either output
 * may be NULL).  A batched call counts its shared prefix once for the single-sequence cache and, per request, the shared
 * tokens as kept and the rest of the prompt as computed. */
void kjarni_hip_decoder_prefix_stats(const KjarniHipDecoder* decoder, uint64_t* reused, uint64_t* computed);
/* Test hook: the tokens whose K / V sit in rows [0, *n) of the single-sequence cache, *n <= cache_len (rows past it belong to
 * tokens a loop computed and discarded); the first min(*n, capacity) are written. */
KjarniErrorCode kjarni_hip_decoder_resident(const KjarniHipDecoder* decoder, uint32_t* out, size_t capacity, size_t* n);
/* Test hook: the logits row [vocab] the last forward of the single-sequence path left on the device (after a generate call
 * with max_new_tokens 0: the logits of the last prompt token). */
KjarniErrorCode kjarni_hip_decoder_last_logits(const KjarniHipDecoder* decoder, float* logits_out);
/* The rule (no GPU, no handle): *keep = min(longest common prefix of resident[n] and prompt[m], limit). */
KjarniErrorCode kjarni_hip_prefix_keep(const uint32_t* resident, size_t n, const uint32_t* prompt, size_t m, size_t limit, size_t* keep);
/* The bookkeeping rule of every generation loop (no GPU, no handle), replayed on a given token stream: a request with a prompt of
 * n_prompt tokens on a cache of `capacity` rows, with max_new_tokens, max_len (0: n_prompt + max_new_tokens) and stop_ids
 * (n_stop 0: default_stop_ids, as a model's eos ids) is offered stream[0], stream[1], ... while it wants a token.  A token is
 * emitted unless it is a stop id; the callback returns false at the cancel_after-th emitted token (-1: never).  *n_emitted:
 * tokens emitted; *n_asked: tokens taken from the stream, the draws a sampled loop would take; *n_fed (may be NULL): emitted
 * tokens that are the input of another step -- never the one the callback refused, nor the one that fills the context; the
 * last of max_new_tokens only with feed_last != 0 (the processor / sampling loops of generate; 0: the lanes). */
KjarniErrorCode kjarni_generation_replay(size_t n_prompt, size_t capacity, size_t max_new_tokens, size_t max_len, const uint32_t* stop_ids,
                                         size_t n_stop, const uint32_t* default_stop_ids, size_t n_default_stop, const uint32_t* stream,
                                         size_t n_stream, int64_t cancel_after, int32_t feed_last, size_t* n_emitted, size_t* n_asked,
                                         size_t* n_fed);
/* Test hook of the lanes' shared prefix (after kjarni_hip_decoder_lanes_begin): rows [0, shared) of the single-sequence cache
 * (shared <= cache_len) are copied into `lane` in one launch, bit for bit, then ids[n] are prefilled behind them. */
KjarniErrorCode kjarni_hip_decoder_lane_prefill_shared(KjarniHipDecoder* decoder, int32_t lane, int32_t shared, const uint32_t* ids,
                                                       int32_t n);
/* The copy kernel alone, host pointers: src [2 * layers, src_floats] (K then V per layer); dst [2 * layers, dst_floats] is read,
 * gets src[c, 0 .. count) at dst[c, dst_offset ..) for every cache c, and is written back.  On the device every source /
 * destination cache starts src_skew / dst_skew floats (0..3) past a 16-byte boundary.  Out-of-range arguments: INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_kv_prefix_copy(int32_t device, const float* src, int32_t layers, int64_t src_floats, int32_t src_skew,
                                             int64_t dst_floats, int32_t dst_skew, int64_t dst_offset, int64_t count, float* dst);
/* Qwen3's per-head RMSNorm + RoPE kernel alone, host pointers: q [q_rows, ldq] and k [k_rows, ldk] are read, `rows` rows are
 * processed in place and both arrays are written back whole.  Row r sits at position pos + r (pos travels in device memory when
 * pos_on_device, as in the captured step); every head vector x [head_dim] of its n_heads Q heads (row r of q) and n_kv_heads K
 * heads (row pos + r of k when k_at_cache_row, else row r) becomes (x / sqrt(mean(x^2) + eps)) * gamma, then its pairs
 * (i, i + head_dim / 2) are rotated by row pos + r of cos_t / sin_t [table_rows, head_dim / 2].  Out-of-range arguments:
 * INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_qk_norm_rope(int32_t device, float* q, int64_t ldq, int32_t q_rows, float* k, int64_t ldk, int32_t k_rows,
                                           int32_t rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const float* gamma_q,
                                           const float* gamma_k, float eps, const float* cos_t, const float* sin_t, int32_t table_rows,
                                           int32_t pos, int32_t pos_on_device, int32_t k_at_cache_row);
/* ---- decoder embedders: last-token pooling over a packed batch -----------------------------------------------------------------
 * kjarni_hip_decoder_embed: sequence b is ids[offsets[b], offsets[b + 1]); out [n_sequences, hidden] receives the final-normed
 * hidden state of every sequence's last token, L2-normalised when `normalize` (x / ||x|| when ||x|| > 0).  The sequences are
 * packed in order into chunks of at most KJARNI_HIP_EMBED_CHUNK_ROWS rows (kjarni_hip_embed_plan) and every chunk runs the
 * prompt routes of kjarni_hip_decoder_forward once over all its rows, with causal attention that stops at the sequence
 * boundaries.  The KV cache, the resident tokens, the lanes, the logits and the last hidden rows are left as they were.
 * INVALID_CONFIG, before any GPU work, naming the argument and the sequence: offsets that decrease, an empty sequence, an
 * id >= vocab, a sequence longer than min(context, KJARNI_HIP_EMBED_CHUNK_ROWS); also for GPT-2 and quantized checkpoints and
 * for hidden / heads * head_dim / intermediate sizes that are no multiple of 32.  n_sequences == 0 is OK and writes nothing. */
#define KJARNI_HIP_EMBED_CHUNK_ROWS 2048
KjarniErrorCode kjarni_hip_decoder_embed(KjarniHipDecoder* decoder, const uint32_t* ids, const int32_t* offsets, int32_t n_sequences,
                                         int32_t normalize, float* out);
/* The packing rule alone (host only).  lengths[n], each 1 .. KJARNI_HIP_EMBED_CHUNK_ROWS (else INVALID_CONFIG naming the entry):
 * sequences go greedily, in order, into chunks of at most KJARNI_HIP_EMBED_CHUNK_ROWS rows and never straddle one.
 * chunk_first_seq (n + 1 entries, may be NULL) receives each chunk's first sequence and, behind the last, n; *n_chunks the count.
 * A sequence of at least 256 rows with head_dim 64 or 128 contributes one block per 128 query rows to the matrix-core table,
 * every other sequence one block per 32 query rows to the vector table; a block is four words (chunk, the sequence's first row
 * in the chunk, the block's first query row in the sequence, the sequence's length).  vec_blocks / mfma_blocks (may be NULL)
 * receive the first vec_capacity / mfma_capacity blocks, *n_vec / *n_mfma the counts. */
KjarniErrorCode kjarni_hip_embed_plan(const int32_t* lengths, int32_t n, int32_t head_dim, int32_t* chunk_first_seq, int32_t* n_chunks,
                                      int32_t* vec_blocks, int32_t vec_capacity, int32_t* n_vec, int32_t* mfma_blocks, int32_t mfma_capacity,
                                      int32_t* n_mfma);
/* The packed attention kernels alone, host pointers.  q [buffer_rows, ldq] (heads * head_dim used), k / v [buffer_rows, ldk / ldv]
 * (kv_heads * head_dim used); sequence b is rows seq_start[b] .. seq_start[b + 1] - 1 (seq_start[0] == 0, increasing,
 * seq_start[n_sequences] <= buffer_rows).  ctx [buffer_rows, ldc] is read, gets the context rows of every sequence (query row r
 * sees the keys of its own sequence up to r) and is written back whole.  head_dim 16 / 32 / 64 / 128, leading dimensions
 * multiples of 4.  Sequences of at least 256 rows with head_dim 64 / 128 run on the matrix-core kernel, the others on the vector
 * kernel, in the same call.  Out-of-range arguments: INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_packed_causal_attention(int32_t device, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                                      int64_t ldv, int32_t buffer_rows, const int32_t* seq_start, int32_t n_sequences,
                                                      int32_t heads, int32_t kv_heads, int32_t head_dim, float* ctx, int64_t ldc);
/* ---- the decode attention and the projections that merge its slabs, alone ---------------------------------------------------------
 * kjarni_hip_op_decode_attention: the split-key attention of every decode step (launch_decode_attention) on host arrays, every
 * argument of the launcher exposed.  q [rows, ldq] (heads * head_dim used).  k / v: k_floats / v_floats floats each, key row t of
 * query row s at k + s * k_lane_stride + t * ldk, KV head h / kv_group at columns [(h / kv_group) * head_dim, + head_dim) (v
 * alike; the lane strides are 0 unless the rows are lanes).  Keys: n_keys; with keys_on_device, n_keys is instead uploaded to a
 * device int and the kernel sees n_keys + rows keys (n_keys + 1 with lanes) and, when causal_base >= 0, the causal base n_keys
 * (max_keys must bound the sum).  causal_base >= 0: query row s sees keys <= causal_base + s; < 0: no mask.  lanes == rows: the
 * rows are independent sequences, no mask.  lane_pos / lane_live [rows] (may be NULL; ragged lanes): row s sees
 * min(lane_pos[s] + 1, n_keys) keys, a row with lane_live[s] == 0 gives zeros.  ctx [rows, ldc] is read, gets the context rows and
 * is written back whole.  slabs (may be NULL) receives the scratch [rows, heads, splits, head_dim + 4] = (max, sum of exp, 0, 0,
 * sum of exp * V) per key range; the scratch is filled with NaN before the launch.  INVALID_CONFIG, before any GPU work, for
 * what the launcher refuses (head_dim not a multiple of 4 that divides 1024 or above 128, splits < 1, more than 512 keys per split,
 * lane_pos without lanes / lane_live or with keys_on_device) and for keys that reach outside k_floats / v_floats, leading
 * dimensions that do not cover the heads or are no multiple of 4, rows outside 1 .. 64. */
KjarniErrorCode kjarni_hip_op_decode_attention(int32_t device, const float* q, int64_t ldq, int32_t rows, const float* k, int64_t k_floats,
                                               int64_t ldk, const float* v, int64_t v_floats, int64_t ldv, int32_t n_keys,
                                               int32_t keys_on_device, int32_t max_keys, int32_t heads, int32_t head_dim, int32_t causal_base,
                                               int32_t splits, int32_t kv_group, int64_t k_lane_stride, int64_t v_lane_stride, int32_t lanes,
                                               const int32_t* lane_pos, const int32_t* lane_live, float* ctx, int64_t ldc, float* slabs);
/* Whisper's one-token output projection fed by attention slabs (launch_gemv_row_att): y [n_out] = merged(slabs) . w[n, :] + bias[n]
 * + r[n]; slabs [k / head_dim, splits, head_dim + 4], w [n_out, k], bias may be NULL.  in_place: the residual row is also the
 * output row on the device, as in the decoder.  two_step: the route the kernel replaces runs instead -- the combine pass, then the
 * one-row projection with bias + residual -- on the same arguments.  INVALID_CONFIG, before any GPU work, for what the launcher
 * refuses: k not 512 / 2048, splits outside 1 .. 16, head_dim no multiple of 4 or not dividing k, r NULL. */
KjarniErrorCode kjarni_hip_op_gemv_row_att(int32_t device, const float* slabs, int32_t splits, int32_t head_dim, const float* w,
                                           const float* bias, const float* r, int32_t n_out, int32_t k, int32_t in_place, int32_t two_step,
                                           float* y);
/* The decoder-only models' output projection fed by attention slabs (launch_llm_gemv with att_splits / att_head_dim): the same
 * inputs, w f32 or bf16 bits (bf16 = 1) [n_out, k], `rows` rows asked of the launcher.  INVALID_CONFIG, before any GPU work, for
 * what the launcher refuses: rows != 1, k 2048 with more than 8 splits, k 4096 with more than 4, any other k, r NULL. */
KjarniErrorCode kjarni_hip_op_llm_gemv_att(int32_t device, const float* slabs, int32_t splits, int32_t head_dim, const void* w, int32_t bf16,
                                           const float* bias, const float* r, int32_t n_out, int32_t k, int32_t rows, float* y);
/* ---- the dense (f32 / bf16) decode-step projections, alone --------------------------------------------------------------------------
 * kjarni_hip_op_llm_gemv: ONE call of launch_llm_gemv (lanes = 0) or launch_llm_gemv_lanes (lanes = 1) on host arrays, every field
 * of the launchers' argument block exposed except the attention slabs (kjarni_hip_op_llm_gemv_att).  Y[r, n] = epi(norm(x[r, :]) .
 * w[n, :] + bias[n]) for `rows` rows.  x [x_rows, ldx] (x_rows >= rows, k columns used).  Norm: gamma [k] (NULL: none) is RMSNorm,
 * x / sqrt(mean(x^2) + eps) * gamma; with layernorm, (x - mean) / sqrt(var + eps) * gamma + beta [k].  w, w2 [n_out, k] f32, or bf16
 * bit patterns with bf16 = 1; bias [n_out] or NULL.  Epilogue: swiglu, silu(x . w + bias) * (x . w2); gelu_tanh (after LayerNorm);
 * residual r [rows, ldr], or with r_is_y0 the output y[0] itself (its stride is then ldy0).  Outputs: seg_q == 0, y[0] [out_rows[0],
 * ldy0] gets row r at row r; seg_q > 0 (seg_q + 2 * seg_kv == n_out), columns [0, seg_q) go to y[0] row r, the next seg_kv to y[1]
 * and the last seg_kv to y[2], both [out_rows[i], ldy12], at row row_off + r.  offset_on_device: row_off is read from device memory
 * and the launcher's by-value copy is another row inside the outputs.  norm_out [k] (may be NULL; one row, gamma, k 2048 / 4096 /
 * 8192): also receives the normalised row.  Every y[i] and norm_out is uploaded as given, written by the kernel and returned
 * whole, so whatever the caller put into rows, padding columns and outputs the call does not own comes back as it was; each has a
 * guard band behind it on the device.  route_out [16] (int32) receives the launcher's own route (llm_gemv_route /
 * llm_gemv_lanes_route, the functions the launchers call): lanes = 0: kernel (0 stream, 1 split-K, 2 one-row LDS, 3 generic), ch,
 * wide, threads, loop, rows_per_batch, workgroups; lanes = 1: taken, ch, ns, wide, cpw, workgroups, streamed (what the launcher
 * reported), and when it fell back, the seven values of the lanes = 0 form from slot 8.  Every operand is uploaded 16-byte aligned:
 * a misaligned w2, which takes K = 2048 off the streaming kernel, cannot be asked for.  INVALID_CONFIG, before any GPU work and with
 * every output untouched: rows outside 0 .. 8 or above x_rows, k % 8, ldx % 4, ldx < k, ldy < the output's columns, ldr < n_out,
 * n_out < 1 or above 2^17, k above 2^16, n_out * k above 2^26, seg_q + 2 * seg_kv != n_out, rows that do not fit an output at
 * row_off, swiglu without w2, and the (epilogue, norm) pairs the launcher rejects: LayerNorm without gamma / beta or with a
 * residual, SwiGLU or norm_out; GELU-tanh without LayerNorm or with segments; SwiGLU without gamma or with a residual; a residual
 * with gamma; norm_out outside its route; an in-place residual with segments. */
KjarniErrorCode kjarni_hip_op_llm_gemv(int32_t device, int32_t lanes, const float* x, int32_t x_rows, int64_t ldx, int32_t rows,
                                       const float* gamma, const float* beta, float eps, int32_t layernorm, int32_t gelu_tanh, const void* w,
                                       const void* w2, int32_t bf16, int32_t swiglu, const float* bias, const float* r, int64_t ldr,
                                       int32_t r_is_y0, int32_t n_out, int32_t k, int32_t seg_q, int32_t seg_kv, float* const* y,
                                       const int32_t* out_rows, int64_t ldy0, int64_t ldy12, int32_t row_off, int32_t offset_on_device,
                                       float* norm_out, int32_t* route_out);
/* kjarni_hip_op_llm_qkv_rope: ONE call of launch_llm_qkv_rope, the one-token RMSNorm + Q | K | V projection + RoPE.  The input row is
 * x [k], or (x NULL) row *embed_ids of table [vocab, k] (the weights' dtype; an id >= vocab gives zeros), which x_raw_out [k] (may
 * be NULL) then also receives.  gamma [k]; w [(n_heads + 2 n_kv_heads) * head_dim, k] f32 or bf16 bit patterns; bias or NULL.
 * cos_t / sin_t [positions, head_dim / 2]; Q and K are rotated on pairs (i, i + head_dim / 2) by row pos.  q [n_heads * head_dim]
 * gets Q; row pos of k_cache / v_cache [cache_rows, n_kv_heads * head_dim] gets K / V.  offset_on_device: pos is read from device
 * memory and the by-value copy is another row.  q, both caches and x_raw_out are uploaded as given and returned whole, with guard
 * bands on the device.  route [3]: kernel (0 a workgroup per pair, 1 streaming, 2 streaming with the gather), ch, workgroups, by
 * llm_qkv_rope_route, which the launcher calls.  INVALID_CONFIG, before any GPU work and with every output untouched: gamma NULL,
 * k % 8 or above 8192, head_dim odd, pos outside the tables or the caches, both or neither of x and embed_ids, a gather without a
 * table or at k other than 2048 / 4096 / 8192, a table or x_raw_out without the gather, sizes above the caps. */
KjarniErrorCode kjarni_hip_op_llm_qkv_rope(int32_t device, const float* x, const uint32_t* embed_ids, const void* table, int32_t vocab,
                                           const float* gamma, float eps, const void* w, int32_t bf16, const float* bias, int32_t k,
                                           int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const float* cos_t, const float* sin_t,
                                           int32_t positions, int32_t pos, int32_t offset_on_device, float* q, float* k_cache, float* v_cache,
                                           int32_t cache_rows, float* x_raw_out, int32_t* route);
/* ---- the Whisper decoder's row projections and the front-end kernels, alone -----------------------------------------------------------
 * kjarni_hip_op_gemv_rows: ONE call of launch_gemv_rows on host arrays, every field of GemvArgs exposed.  Y[r, n] = epi(LN?(x[r, :])
 * . w[n, :] + bias[n]) (+ R[r, n]) for `rows` rows.  x [x_rows, ldx] (NULL with embed_id); gamma, beta [k] (gamma given: LayerNorm,
 * (x - mean) / sqrt(var + eps) * gamma + beta); w [n_out, k]; bias [n_out] or NULL; epi: 0 bias, 1 erf GELU, 5 residual -- r [rows,
 * ldr], or with r_is_y0 the output y[0] itself, as the decoder calls it.  seg == 0: y[0] [out_rows[0], ldy0] gets row r at row r;
 * seg > 0: columns [0, seg) go to y[0] row r, [seg, 2 seg) to y[1] and [2 seg, 3 seg) to y[2], both [out_rows[i], ldy12], at row
 * row_off + r.  offset_on_device: row_off is read from device memory and the launcher's by-value copy is another row inside the
 * outputs.  embed_id (one id, or NULL): the kernel builds its input row as embed_word [embed_vocab, k] row id * embed_scale +
 * embed_pos_table [embed_max_pos, k] (or NULL) row embed_pos -- zeros for an id or a position outside its table;
 * embed_pos_on_device as offset_on_device.  x_raw_out [k] (or NULL; with embed_id): the row as built; x_norm_out [k] (or NULL; with
 * gamma): the row after the LayerNorm.
 * misalign: a mask (1 x, 2 w, 4 gamma, 8 beta) of operands uploaded 4 bytes past a 16-byte boundary.  Every y[i], x_raw_out and
 * x_norm_out is uploaded as given, written by the kernel and returned whole, with a guard band behind it on the device.
 * *route_out: gemv_rows_route's answer, which the launcher follows: 0 nothing to do (rows or n_out <= 0), 1 one-row fast, 2 one-row
 * fast + embed, 3 staged fast, 4 head, 5 staged, 6 general, 7 GEMM.  INVALID_CONFIG, before any GPU work and with every output
 * untouched: sizes outside the caps, ldx < k, ldy < the output's columns, ldr < n_out, rows that do not fit an output at row_off,
 * an in-place residual with segments, embed fields without embed_id -- and everything the launcher's rule refuses (route 8):
 * LayerNorm without beta, a residual epilogue without a residual, an (epilogue, LayerNorm) pair outside the four, n_out above
 * 3 seg, the embed or x_raw_out / x_norm_out outside the one-row kernel, x_raw_out without embed_id, x_norm_out without gamma,
 * gamma or segments on the GEMM route. */
KjarniErrorCode kjarni_hip_op_gemv_rows(int32_t device, const float* x, int32_t x_rows, int64_t ldx, int32_t rows, const float* gamma,
                                        const float* beta, float eps, const float* w, const float* bias, const float* r, int64_t ldr,
                                        int32_t r_is_y0, int32_t n_out, int32_t k, int32_t seg, float* const* y, const int32_t* out_rows,
                                        int64_t ldy0, int64_t ldy12, int32_t row_off, int32_t offset_on_device, int32_t epi,
                                        const uint32_t* embed_id, const float* embed_word, int32_t embed_vocab, const float* embed_pos_table,
                                        int32_t embed_max_pos, int32_t embed_pos, int32_t embed_pos_on_device, float embed_scale,
                                        float* x_raw_out, float* x_norm_out, int32_t misalign, int32_t* route_out);
/* gemv_rows_route alone, no device needed: the route (0 .. 8 as above) for arguments given as sizes and flags; every pointer the
 * rule tests is made non-NULL where its flag is set and 16-byte aligned unless `misalign` (the mask above) shifts it. */
KjarniErrorCode kjarni_hip_gemv_rows_route(int32_t rows, int32_t n_out, int32_t k, int64_t ldx, int32_t seg, int32_t epi, int32_t has_gamma,
                                           int32_t has_beta, int32_t has_r, int32_t embed, int32_t x_raw_out, int32_t x_norm_out,
                                           int32_t misalign, int32_t* route_out);
/* The Whisper front-end kernels, one launch per call on host arrays; every output is uploaded as given and returned whole, with a
 * guard band behind it.  INVALID_CONFIG before any GPU work for sizes outside the caps or a stride that does not cover its row.
 * mel_frames: frames [n_frames, ld] = the signal reflect-padded by n_fft / 2, framed every `hop` samples and windowed; columns
 *   >= n_fft and frames past the padded end are zero.
 * mel_power: power [n_frames, ld_out] = sqrt(re^2 + im^2)^2, re at column k and im at column im_off + k of dft [n_frames, ld_dft];
 *   columns >= n_bins are zero.
 * mel_log_normalize: mel [n_frames, ld] becomes log10(max(mel, 1e-10)) over its first n_mels columns; out [n_frames, ld_out] =
 *   (max(log, max log - 8) + 4) / 4.
 * im2col3: cols [t_out, ld_cols], column j * channels + c = x [t * stride + j - pad, c] (zero outside [0, t_in), zero from column
 *   3 * channels on); x [t_in, ldx].
 * add_rows: x [rows, hidden] += table [r % period] where r % period < table_rows; table [table_alloc_rows, hidden].
 * decoder_embed: out [n, hidden] = word [ids[s]] * (sqrt(hidden) with scale_embeddings) + pos [offset + s] (lanes: offset for every
 *   row); zeros for ids >= vocab, nothing added for positions >= max_pos; pos may be NULL; offset_on_device as above. */
KjarniErrorCode kjarni_hip_op_mel_frames(int32_t device, const float* audio, int64_t n_samples, const float* window, int32_t n_fft,
                                         int32_t hop, int32_t n_frames, int32_t ld, float* frames);
KjarniErrorCode kjarni_hip_op_mel_power(int32_t device, const float* dft, int32_t ld_dft, int32_t im_off, int32_t n_bins, int32_t ld_out,
                                        int32_t n_frames, float* power);
KjarniErrorCode kjarni_hip_op_mel_log_normalize(int32_t device, float* mel, int32_t ld, int32_t n_mels, int32_t n_frames, int32_t ld_out,
                                                float* out);
KjarniErrorCode kjarni_hip_op_im2col3(int32_t device, const float* x, int64_t ldx, int32_t t_in, int32_t channels, int32_t stride,
                                      int32_t pad, int32_t t_out, int32_t ld_cols, float* cols);
KjarniErrorCode kjarni_hip_op_add_rows(int32_t device, float* x, int32_t rows, int32_t hidden, int32_t period, const float* table,
                                       int32_t table_rows, int32_t table_alloc_rows);
KjarniErrorCode kjarni_hip_op_decoder_embed(int32_t device, const uint32_t* ids, int32_t n, int32_t hidden, int32_t vocab, const float* word,
                                            const float* pos, int32_t max_pos, int32_t offset, int32_t offset_on_device,
                                            int32_t scale_embeddings, int32_t lanes, float* out);
/* ---- the encoder's packed-row kernels, alone ----------------------------------------------------------------------------------------
 * A ragged batch runs over its kept tokens only: sentence b is rows cu[b] .. cu[b+1] of every activation buffer and tok_src[row] is
 * the row's index in the padded [batch, seq] arrays.  Each hook below makes ONE launcher call on host arrays.  Every argument is
 * checked before a device is asked for (INVALID_CONFIG / NULL_POINTER with the outputs untouched); every output is uploaded as given
 * and returned whole, so what the kernel does not own keeps the caller's pattern; a guard band lies behind every device buffer
 * (128 rows behind qkv, ctx and the hidden states), checked behind outputs and NaN behind inputs.
 *
 * mask_lengths: lens_out[b] = kept tokens (mask != 0) of sentence b of mask [batch, seq]; bit 31 set when mask[b, 0] == 0 or a mask
 *   value is > 1 (the sentence needs the padded layout).
 * pack_index: tok_src[cu[b] + r] = b * seq + s for the r-th kept token of sentence b; tok_src [capacity] otherwise untouched.  The
 *   kernel writes tok_src + cu[b] unchecked, so the hook refuses a cu that does not start at 0, decreases, whose steps are not the
 *   mask's kept counts, or that ends beyond capacity.
 * encoder_embed: launch_embed_layernorm.  out [rows, hidden]: row t = token tok_src[t] (t without tok_src) of ids / type_ids
 *   [batch, seq]: word [id] (zeros when id >= vocab) * sqrt(hidden) with scale_embeddings, + pos [pos_offset + s] when that is below
 *   max_pos, + type [type id] (row 0 without type_ids); LayerNorm(gamma, beta, eps) when gamma is given.  pos, type, type_ids, gamma /
 *   beta and tok_src may be NULL.  Refused: tok_src[t] outside [0, batch * seq), a type id >= type_vocab, gamma without beta, pos with
 *   max_pos <= 0, rows > batch * seq without tok_src.
 * encoder_rope: launch_rope_qk on qkv [rows, 3 * heads * head_dim] in place (the V third untouched); position of row t =
 *   tok_src[t] % seq (t % seq without); cos_t / sin_t [seq, head_dim].  Refused: odd head_dim, a negative tok_src entry.
 * attention_packed: launch_attention(..., cu) on qkv [buffer_rows, 3 hidden] -> ctx [buffer_rows, hidden]; max_len = the longest
 *   sentence the call is sized for.  Refused: a cu that is not strictly increasing from 0 (the kernels compute extents from len - 1),
 *   a sentence longer than max_len (the grids cover max_len queries: a caller's precondition of launch_attention), cu[batch] >
 *   buffer_rows.  route_out [2] = the kernel (KjarniHipAttentionKernel) and the item-per-workgroup kernels' grid, as
 *   kjarni_hip_attention_route gives them.
 * pool_packed: launch_pool(..., cu) on hidden_states [cu[batch], hidden] -> out [batch, hidden]; the same cu checks against `seq`;
 *   hidden <= 1024.  (launch_pool ignores a mask when cu is given: every packed row is a kept token.)
 * small_linear: out [rows, n] = feat [rows, ld] (the first k of every row) . w [n, k]^T + bias [n] (NULL: none).
 * row_softmax: out [rows, n] = softmax of every row of in, or 1 / (1 + exp(-x)) per element with sigmoid.
 * attention_route: host only, no device.  Which kernel launch_attention takes for (batch, seq or longest sentence, heads, head_dim),
 *   `aligned` = hidden % 4 == 0 and 16-byte aligned buffers, `packed` = cu given; route_out [2] as above. */
typedef enum {
    KJARNI_HIP_ATTN_NOTHING = 0,     /* batch <= 0 or seq <= 0 */
    KJARNI_HIP_ATTN_SPLIT = 1,       /* the small-call kernel: at most 128 (sentence, head) items, seq <= 128 */
    KJARNI_HIP_ATTN_PIPE_PADDED = 2, /* item per workgroup, MODE 0: padded rows, 96 < seq <= 128 */
    KJARNI_HIP_ATTN_PIPE_PACKED = 3, /* item per workgroup, MODE 1: packed rows, longest sentence <= 128 */
    KJARNI_HIP_ATTN_PIPE_SHORT = 4,  /* item per workgroup, MODE 2: padded rows, seq <= 96 */
    KJARNI_HIP_ATTN_CHUNKED = 5,     /* seq > 128: online softmax over chunks of 128 keys */
    KJARNI_HIP_ATTN_GENERIC = 6      /* head_dim other than 32 / 64, or not aligned */
} KjarniHipAttentionKernel;
KjarniErrorCode kjarni_hip_op_mask_lengths(int32_t device, const uint32_t* mask, int64_t batch, int32_t seq, uint32_t* lens_out);
KjarniErrorCode kjarni_hip_op_pack_index(int32_t device, const uint32_t* mask, const int32_t* cu, int64_t batch, int32_t seq,
                                         int32_t* tok_src, int32_t capacity);
KjarniErrorCode kjarni_hip_op_encoder_embed(int32_t device, const uint32_t* ids, const uint32_t* type_ids, const float* word, const float* pos,
                                            const float* type, const float* gamma, const float* beta, float eps, int64_t rows, int64_t batch,
                                            int32_t seq, int32_t hidden, int32_t vocab, int32_t max_pos, int32_t type_vocab, int32_t pos_offset,
                                            int32_t scale_embeddings, const int32_t* tok_src, float* out);
KjarniErrorCode kjarni_hip_op_encoder_rope(int32_t device, float* qkv, const float* cos_t, const float* sin_t, int64_t rows, int32_t seq,
                                           int32_t heads, int32_t head_dim, const int32_t* tok_src);
KjarniErrorCode kjarni_hip_op_attention_packed(int32_t device, const float* qkv, const int32_t* cu, int64_t batch, int32_t max_len,
                                               int32_t heads, int32_t head_dim, float mask_value, float* ctx, int64_t buffer_rows,
                                               int32_t* route_out);
KjarniErrorCode kjarni_hip_op_pool_packed(int32_t device, const float* hidden_states, const int32_t* cu, int64_t batch, int32_t seq,
                                          int32_t hidden, KjarniHipPooling pooling, int32_t normalize, float* out);
KjarniErrorCode kjarni_hip_op_small_linear(int32_t device, const float* feat, int64_t ld, const float* w, const float* bias, int64_t rows,
                                           int32_t k, int32_t n, float* out);
KjarniErrorCode kjarni_hip_op_row_softmax(int32_t device, const float* in, int64_t rows, int32_t n, int32_t sigmoid, float* out);
KjarniErrorCode kjarni_hip_attention_route(int64_t batch, int32_t seq_or_max_len, int32_t heads, int32_t head_dim, int32_t aligned,
                                           int32_t packed, int32_t* route_out);
/* ---- the prompt-route GEMM and the two prefill attention kernels, alone -------------------------------------------------------------
 * kjarni_hip_op_prefill_gemm: y[m, n] = a[m, k] . w[n, k]^T (+ bias) (+ r) through launch_prefill_gemm (64 x 64 tiles, K slices
 * added by the reduce kernel), as the decoders' prompt projections call it.  a [a_rows, lda] (a_rows >= m, lda >= k); w [n, k] f32,
 * or bf16 bit patterns with bf16 = 1; bias [n] or NULL.  Residual: r [m, ldr] (NULL: none), or with r_is_y the output itself
 * (r and ldr are then ignored and the residual's stride is ldy).  y [m, ldy] is read, gets the result and is written back whole.
 * gate [m, n] (may be NULL) is read and becomes silu(gate) * (the product); with a K split y is then left as it was, without one
 * y also holds the product.  split: 0 passes the launcher no scratch, 1 a scratch of prefill_gemm_scratch_floats() floats filled
 * with NaN (all-ones words) before the launch; *scratch_written (may be NULL; needs split) receives the number of scratch words
 * that no longer hold that pattern.  *ksplit_used: the number of K slices the launcher took (1, 2, 4 or 8; by the launcher's own
 * rule).  INVALID_CONFIG, before any GPU work and with every output untouched: k % 32, lda % 4, m < 0 or above 4096, n or k < 1
 * (n above 2^17, k above 2^16, n * k above 2^26), a gate with ldy != n or n % 4, lda < k, ldy < n, a residual with ldr < n. */
KjarniErrorCode kjarni_hip_op_prefill_gemm(int32_t device, const float* a, int64_t lda, int32_t a_rows, const void* w, int32_t bf16,
                                           const float* bias, const float* r, int64_t ldr, int32_t r_is_y, float* y, int64_t ldy, float* gate,
                                           int32_t m, int32_t n, int32_t k, int32_t split, int32_t* ksplit_used, int64_t* scratch_written);
/* kjarni_hip_op_prefill_gemm_fp8: the same call through launch_prefill_gemm_fp8 -- the weights as FP8 (e4m3fn) codes [n, k], one
 * byte each, with scale [scale_rows, scale_cols] of shape [1, 1] (per tensor), [n, 1] (per channel) or [ceil(n / 128), k / 128]
 * (128 x 128 blocks): y = a . (decode(code) * scale)^T (+ bias) (+ r), the codes decoded in the tile loader and multiplied on the
 * bf16 matrix cores, the scale applied in f32.  Every other argument, the split scratch, *ksplit_used and *scratch_written as in
 * kjarni_hip_op_prefill_gemm; a guard band lies behind every device buffer and the outputs come back whole.  INVALID_CONFIG, before
 * any GPU work and with every output untouched: the refusals of kjarni_hip_op_prefill_gemm, a scale shape that fits no kind, a NaN
 * code (0x7F, 0xFF). */
KjarniErrorCode kjarni_hip_op_prefill_gemm_fp8(int32_t device, const float* a, int64_t lda, int32_t a_rows, const void* codes, const float* scale,
                                               int32_t scale_rows, int32_t scale_cols, const float* bias, const float* r, int64_t ldr,
                                               int32_t r_is_y, float* y, int64_t ldy, float* gate, int32_t m, int32_t n, int32_t k, int32_t split,
                                               int32_t* ksplit_used, int64_t* scratch_written);
/* kjarni_hip_op_prefill_attention: causal grouped-query attention of `rows` prompt rows at positions base .. base + rows - 1 over
 * key rows 0 .. base + rows - 1 through launch_prefill_attention: query row s sees keys <= base + s.  q [rows, ldq]
 * (heads * head_dim used); k / v: k_floats / v_floats floats, key row t at k + t * ldk, KV head h / kv_group at columns
 * [(h / kv_group) * head_dim, + head_dim).  ctx [rows, ldc] is read, gets the context rows and is written back whole.  *route: the
 * kernel the launcher took, 0 the vector kernel, 1 the matrix-core kernel (blocks of at least 256 rows at head_dim 64 / 128).
 * INVALID_CONFIG, before any GPU work and with every output untouched: head_dim not 16 / 32 / 64 / 128, rows < 1, base < 0,
 * kv_group < 1 or not dividing heads, leading dimensions that are no multiple of 4 or do not cover the heads, key rows that reach
 * outside k_floats / v_floats. */
KjarniErrorCode kjarni_hip_op_prefill_attention(int32_t device, const float* q, int64_t ldq, int32_t rows, const float* k, int64_t k_floats,
                                                int64_t ldk, const float* v, int64_t v_floats, int64_t ldv, int32_t base, int32_t heads,
                                                int32_t head_dim, int32_t kv_group, float* ctx, int64_t ldc, int32_t* route);
/* ---- wide lanes: the per-lane kernels of the wide step, alone ---------------------------------------------------------------------
 * KjarniHipWideState: what the wide step keeps on the device per lane -- the next input token, the position (= the lane's cache
 * length), live (0: frozen, nothing of the lane is read or written), the picks so far, the picks after which the lane is done,
 * and its stop ids.  kjarni_hip_wide_state_size() = sizeof of the native struct (a binding checks its mirror against it). */
#define KJARNI_HIP_WIDE_LANES 64
#define KJARNI_HIP_LANE_STOPS 16
typedef struct KjarniHipWideState {
    int32_t token[KJARNI_HIP_WIDE_LANES];
    int32_t pos[KJARNI_HIP_WIDE_LANES];
    int32_t live[KJARNI_HIP_WIDE_LANES];
    int32_t count[KJARNI_HIP_WIDE_LANES];
    int32_t limit[KJARNI_HIP_WIDE_LANES];
    int32_t n_stop[KJARNI_HIP_WIDE_LANES];
    int32_t stop[KJARNI_HIP_WIDE_LANES][KJARNI_HIP_LANE_STOPS];
} KjarniHipWideState;
size_t kjarni_hip_wide_state_size(void);
/* kjarni_hip_op_wide_rope_scatter: ONE call of launch_wide_rope_scatter (gamma_q and gamma_k NULL) or of
 * launch_wide_qk_norm_rope_scatter (both given: Qwen3's per-head RMSNorm of Q and K before the rotation).  Row `lane` of qkv
 * [lanes, ld] holds Q | K | V of the lane's new token: Q is rotated in place at pos[lane]; K is rotated (rotate == 0: copied) and V
 * copied to row pos[lane] of k_cache / v_cache + lane * lane_stride.  A lane with live == 0 or pos >= capacity writes nothing.
 * qkv, k_cache and v_cache [lanes, lane_stride] are read and written back whole, each behind a guard band.  cos_t / sin_t
 * [table_rows, head_dim / 2].  INVALID_CONFIG, before any GPU work and with every output untouched: lanes outside 1..64,
 * head_dim odd or outside 2..128, n_kv_heads above n_heads, ld short of Q | K | V, lane_stride short of capacity rows, a
 * negative position, a live position inside the capacity but outside the tables, one gamma without the other, the Qwen3 form
 * with rotate == 0. */
KjarniErrorCode kjarni_hip_op_wide_rope_scatter(int32_t device, float* qkv, int64_t ld, int32_t lanes, int32_t n_heads, int32_t n_kv_heads,
                                                int32_t head_dim, const float* gamma_q, const float* gamma_k, float eps, const float* cos_t,
                                                const float* sin_t, int32_t table_rows, float* k_cache, float* v_cache, int64_t lane_stride,
                                                int32_t capacity, const int32_t* pos, const int32_t* live, int32_t rotate);
/* kjarni_hip_op_wide_pick: ONE call of launch_wide_pick over lanes [first_lane, first_lane + lanes) of logits
 * [first_lane + lanes, ld]: for every live lane the argmax (the last maximum wins, +0 == -0, NaN lowest) is appended to
 * history[lane * hist_stride + count], count (and pos when advance) + 1, live cleared on a stop id, at count == limit or at
 * pos >= capacity, else token = the pick.  state and history [64, hist_stride] are read and written back whole.
 * INVALID_CONFIG, before any GPU work and with every output untouched: lanes outside 0..64, ld < vocab, hist_stride < 1,
 * n_stop outside 0..16, a live lane whose count is no entry of its history. */
KjarniErrorCode kjarni_hip_op_wide_pick(int32_t device, const float* logits, int64_t ld, int32_t vocab, int32_t lanes, int32_t first_lane,
                                        KjarniHipWideState* state, int32_t* history, int32_t hist_stride, int32_t capacity, int32_t advance);
/* ---- mixture-of-experts (qwen3_moe): the router pick and the sparse FFN, alone ------------------------------------------------------
 * kjarni_hip_op_moe_route: softmax over the E router logits of each row, the k largest (on equal logits the lower expert first),
 * with norm_topk the k weights divided by their sum.  logits [rows, E]; ids_out [rows, k] (int32), weights_out [rows, k], slot 0
 * the largest.  INVALID_CONFIG, before any GPU work and with every output untouched: E outside 2 .. 256, k outside 1 .. 8 or
 * above E, rows outside 1 .. 2^20. */
KjarniErrorCode kjarni_hip_op_moe_route(int32_t device, const float* logits, int32_t rows, int32_t E, int32_t k, int32_t norm_topk,
                                        int32_t* ids_out, float* weights_out);
/* kjarni_hip_op_moe_ffn: y = r + sum_j w_j * down_{e_j}( silu(gate_{e_j} xn) * (up_{e_j} xn) ), xn = RMSNorm(x, gamma, eps) (gamma
 * NULL: x as it is), experts and weights by the route of xn . router^T, summed in slot order j = 0 .. k - 1.  x [rows, ldx]
 * (`hidden` used); router [E, hidden], gate / up [E, Im, hidden], down [E, hidden, Im], f32 or bf16 bit patterns (bf16 = 1).
 * Residual: r [rows, ldr], or with r_is_y the output itself (r and ldr are then ignored).  y [rows, ldy] is read, gets the result
 * and is written back whole.  route: 0 the decoders' rule (fewer than 24 rows: the steps kernels in blocks of 8 rows, else the
 * grouped kernels), 1 the steps kernels, 2 the grouped kernels; *route_used gets 1 or 2, *tiles_used the number of non-empty
 * 64-slot tiles of the grouped plan (0 on the steps route).  ids_out / weights_out [rows, k]: what the router chose.
 * INVALID_CONFIG, before any GPU work and with every output untouched: E outside 2 .. 256, k outside 1 .. 8 or above E, Im % 32,
 * hidden % 32 or above 8192, k * Im above 16384, rows outside 1 .. 4096, a stack above 2^27 elements, a leading dimension that is
 * no multiple of 4 or does not cover hidden, route outside 0 .. 2, no residual. */
KjarniErrorCode kjarni_hip_op_moe_ffn(int32_t device, const float* x, int64_t ldx, int32_t rows, const float* gamma, float eps,
                                      const void* router, const void* gate, const void* up, const void* down, int32_t bf16, int32_t hidden,
                                      int32_t E, int32_t k, int32_t Im, int32_t norm_topk, const float* r, int64_t ldr, int32_t r_is_y, float* y,
                                      int64_t ldy, int32_t route, int32_t* ids_out, float* weights_out, int32_t* route_used,
                                      int32_t* tiles_used);
/* kjarni_hip_decoder_moe_routing: what sparse layer `layer` of a qwen3_moe decoder chose in its last pass (a decode step: 1 row;
 * a verify block or a lane step: its rows; a prompt chunk or a packed pass: its rows, at most 2048).  *rows gets the number of
 * rows recorded; ids_out / weights_out (each may be NULL to ask for the count alone; capacity rows_capacity * k) get [rows, k].
 * INVALID_CONFIG for a dense layer, a dense model, a layer out of range or a capacity below the rows recorded. */
KjarniErrorCode kjarni_hip_decoder_moe_routing(KjarniHipDecoder* decoder, int32_t layer, int32_t rows_capacity, int32_t* rows, int32_t* ids_out,
                                               float* weights_out);
/* RoPE alone, host pointers: x [x_rows, ldx] is read, its first `rows` rows (n_heads heads of head_dim) are rotated in place and
 * it is written back whole.  kjarni_hip_op_rope: row r by table row pos + r (the kernel of the prompt and decode paths);
 * kjarni_hip_op_rope_rows: row r by table row row_pos[r].  cos_t / sin_t [table_rows, head_dim / 2].  Positions outside the
 * tables: INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_rope(int32_t device, float* x, int64_t ldx, int32_t x_rows, int32_t rows, int32_t n_heads, int32_t head_dim,
                                   const float* cos_t, const float* sin_t, int32_t table_rows, int32_t pos);
KjarniErrorCode kjarni_hip_op_rope_rows(int32_t device, float* x, int64_t ldx, int32_t x_rows, int32_t rows, int32_t n_heads, int32_t head_dim,
                                        const float* cos_t, const float* sin_t, int32_t table_rows, const int32_t* row_pos);
/* kjarni_hip_op_qk_norm_rope with row r at position row_pos[r] (its K heads are row r of k). */
KjarniErrorCode kjarni_hip_op_qk_norm_rope_rows(int32_t device, float* q, int64_t ldq, int32_t q_rows, float* k, int64_t ldk, int32_t k_rows,
                                                int32_t rows, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim, const float* gamma_q,
                                                const float* gamma_k, float eps, const float* cos_t, const float* sin_t, int32_t table_rows,
                                                const int32_t* row_pos);
/* The last-token pool alone, host pointers: x [x_rows, ldx]; out [n_sequences, hidden] receives, for every sequence, row
 * seq_start[b + 1] - 1 of x through (x / sqrt(mean(x^2) + eps)) * gamma and, when `normalize`, divided by its L2 norm when that is
 * > 0.  seq_start increasing from >= 0, seq_start[n_sequences] <= x_rows, hidden 1 .. 16384. */
KjarniErrorCode kjarni_hip_op_last_token_pool(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* seq_start,
                                              int32_t n_sequences, int32_t hidden, const float* gamma, float eps, int32_t normalize,
                                              float* out);
/* ---- scoring many sequences in one packed pass ------------------------------------------------------------------------------------
 * kjarni_hip_decoder_score_batch: kjarni_hip_decoder_score / _score_topk for n_sequences sequences at once.  Sequence b is
 * ids[offsets[b], offsets[b + 1]) and its scored positions are [firsts[b], len_b), 1 <= firsts[b] < len_b.  The outputs are flat, in
 * sequence order then position order: logprob_out [S], S = sum(len_b - firsts[b]); topk_ids_out / topk_logprob_out [S, top_k]
 * row-major (top_k 1 .. KJARNI_SCORE_TOPK_MAX, not above the vocabulary; slot 0 is kjarni_hip_decoder_score's top /
 * top_logprob).  Any output may be NULL.  The sequences are packed in order into chunks of at most KJARNI_HIP_EMBED_CHUNK_ROWS
 * rows (kjarni_hip_score_plan) and every chunk runs kjarni_hip_decoder_embed's layer stack once over its rows; a token prefix that
 * neighbouring sequences share -- never a scored token -- is computed once, and only the rows whose successor is scored reach the
 * vocabulary head, on kjarni_hip_decoder_score's routes (counted by kjarni_hip_decoder_score_calls).  Sharing is decided from the
 * input alone.  The KV cache, the resident tokens, the lanes, the logits, the last hidden rows, the prefix-reuse counters and the
 * buffers of kjarni_hip_decoder_score are left as they were.  INVALID_CONFIG, before any GPU work, naming the argument and the
 * sequence: offsets that decrease, a sequence shorter than 2 or longer than min(context, KJARNI_HIP_EMBED_CHUNK_ROWS), firsts[b]
 * out of range, an id >= vocab, top_k out of range; also for quantized checkpoints and for hidden / heads * head_dim /
 * intermediate sizes that are no multiple of 32 (GPT-2 is accepted).  n_sequences == 0 is OK and writes nothing. */
#define KJARNI_HIP_SCORE_MIN_SHARED 2 /* the shortest shared prefix kjarni_hip_decoder_score_batch computes once (its plan's min_shared) */
KjarniErrorCode kjarni_hip_decoder_score_batch(KjarniHipDecoder* decoder, const uint32_t* ids, const int32_t* offsets, int32_t n_sequences,
                                               const int32_t* firsts, int32_t top_k, float* logprob_out, uint32_t* topk_ids_out,
                                               float* topk_logprob_out);
/* Rows kjarni_hip_decoder_score_batch computed, and prefix rows it did not compute a second time (the sum of (members - 1) *
 * prefix over its groups), since load (zeros on NULL; either output may be NULL). */
void kjarni_hip_decoder_score_batch_rows(const KjarniHipDecoder* decoder, uint64_t* computed, uint64_t* saved);
/* The plan alone (host only).  Walking the sequences in order, sequence i gathers the neighbours behind it while the prefix
 * q = min(prefix so far, firsts[j], common prefix of i and j) stays >= min_shared (>= 1), the group's rows q + sum(len - q) fit
 * KJARNI_HIP_EMBED_CHUNK_ROWS and every remainder len - q stays below 256 rows; two or more members form a group (its prefix
 * rows first, then each remainder), else sequence i stays plain.  Units go greedily, in order, into chunks and never straddle
 * one.  chunk_first_seq (n + 1 entries, may be NULL): each chunk's first sequence and, behind the last, n; chunk_rows (n entries,
 * may be NULL): each chunk's rows; groups [capacity, 4]: (chunk, first sequence, members, prefix length).  Prefixes and plain
 * sequences get their blocks by kjarni_hip_embed_plan's rule into vec_blocks / mfma_blocks [capacity, 4] (chunk, first row, the
 * block's first query row, length); every remainder gets one block per 32 query rows in prefix_blocks [capacity, 6] (chunk, the
 * remainder's first row, the block's first query row in the remainder, the remainder's length, the prefix's first row, the
 * prefix length).  gather [capacity, 4]: for every scored position pos, in sequence order then position order, (chunk, the chunk
 * row of position pos - 1 -- the prefix's last row when pos - 1 is its last token --, the target id, the slot in the flat
 * outputs).  Every table may be NULL; the counts are always written.  INVALID_CONFIG naming the argument and the sequence for
 * offsets that decrease, a length outside 2 .. KJARNI_HIP_EMBED_CHUNK_ROWS and firsts[b] outside [1, len_b). */
KjarniErrorCode kjarni_hip_score_plan(const uint32_t* ids, const int32_t* offsets, const int32_t* firsts, int32_t n, int32_t head_dim,
                                      int32_t min_shared, int32_t* chunk_first_seq, int32_t* chunk_rows, int32_t* n_chunks, int32_t* groups,
                                      int32_t group_capacity, int32_t* n_groups, int32_t* vec_blocks, int32_t vec_capacity, int32_t* n_vec,
                                      int32_t* mfma_blocks, int32_t mfma_capacity, int32_t* n_mfma, int32_t* prefix_blocks,
                                      int32_t prefix_capacity, int32_t* n_prefix, int32_t* gather, int32_t gather_capacity, int32_t* n_gather);
/* The prefix attention kernel alone, host pointers; q / k / v / ctx as kjarni_hip_op_packed_causal_attention takes them.
 * remainders [n_remainders, 4]: (first row, rows, the prefix's first row, prefix rows).  The query at row t of a remainder sees
 * the prefix rows and the remainder's rows 0 .. t; its context row is what kjarni_hip_op_packed_causal_attention's vector kernel
 * gives for row prefix + t of the concatenation, bit for bit.  ctx is read and written back whole.  INVALID_CONFIG: rows outside
 * the buffer, a prefix that overlaps its remainder, head_dim not 16 / 32 / 64 / 128, leading dimensions that are no multiple of 4. */
KjarniErrorCode kjarni_hip_op_packed_prefix_attention(int32_t device, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                                      int64_t ldv, int32_t buffer_rows, const int32_t* remainders, int32_t n_remainders,
                                                      int32_t heads, int32_t kv_heads, int32_t head_dim, float* ctx, int64_t ldc);
/* The gather + final norm alone, host pointers: out[j, 0 .. hidden) = norm(x[src[j], :]) for j < n, out rows ldo floats apart (ldo a
 * multiple of 4; out is read and written back whole).  beta NULL: (x / sqrt(mean(x^2) + eps)) * gamma, bit for bit
 * kjarni_hip_op_last_token_pool without normalisation on the same rows; beta given: LayerNorm, bit for bit kjarni_hip_op_layer_norm
 * on the gathered rows.  src[j] outside [0, x_rows): INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_score_gather_norm(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* src, int32_t n,
                                                int32_t hidden, const float* gamma, const float* beta, float eps, float* out, int64_t ldo);
/* ---- answer logits: a few chosen logits at the end of many sequences ---------------------------------------------------------------
 * kjarni_hip_decoder_answer_logits: logits_out[b, t] (row-major [n_sequences, n_targets]) is the logit of token targets[t] at the
 * position after the last token of sequence b = ids[offsets[b], offsets[b + 1]): the dot product of the final-normed last hidden
 * row with row targets[t] of the (tied or untied, f32 or bf16) head.  The targets, 1 .. KJARNI_HIP_ANSWER_MAX_TARGETS of them, are
 * shared by the batch: two for a yes / no reranker (kjarni_reranker_* on a decoder checkpoint), up to eight for multiple choice
 * by answer letter.  The sequences are packed as kjarni_hip_decoder_score_batch packs them (kjarni_hip_answer_plan); a token prefix
 * that neighbouring sequences share -- never with a sequence's last token in it -- is computed once, and the vocabulary head does
 * not run: one kernel reads the last rows and the targeted head rows.  The KV cache, the resident tokens, the lanes, the logits,
 * the last hidden rows, the prefix-reuse counters and the buffers and counters of kjarni_hip_decoder_score / _score_batch are left
 * as they were.  INVALID_CONFIG, before any GPU work, naming the argument and the sequence: offsets that decrease, a sequence
 * shorter than 2 or longer than min(context, KJARNI_HIP_EMBED_CHUNK_ROWS), an id or a target >= vocab, n_targets out of range;
 * also for quantized checkpoints and for hidden / heads * head_dim / intermediate sizes that are no multiple of 32 (GPT-2 is
 * accepted).  n_sequences == 0 is OK and writes nothing. */
#define KJARNI_HIP_ANSWER_MAX_TARGETS 8
KjarniErrorCode kjarni_hip_decoder_answer_logits(KjarniHipDecoder* decoder, const uint32_t* ids, const int32_t* offsets, int32_t n_sequences,
                                                 const uint32_t* targets, int32_t n_targets, float* logits_out);
/* Rows kjarni_hip_decoder_answer_logits computed, and prefix rows it did not compute a second time, since load (zeros on NULL;
 * either output may be NULL).  kjarni_hip_decoder_score_batch_rows counts its own calls only. */
void kjarni_hip_decoder_answer_rows(const KjarniHipDecoder* decoder, uint64_t* computed, uint64_t* saved);
/* The plan alone (host only): kjarni_hip_score_plan's rule and tables with firsts[b] = len_b - 1, so that no prefix holds a
 * sequence's last token -- two identical sequences share all but their last token, and a sequence that is a prefix of its
 * neighbour shares all but its own last token.  gather [capacity, 3]: for every sequence, in order, (chunk, the chunk row of its
 * last token, the sequence's index = its row in logits_out).  Every table may be NULL; the counts are always written.
 * INVALID_CONFIG naming the argument and the sequence for offsets that decrease and a length outside 2 ..
 * KJARNI_HIP_EMBED_CHUNK_ROWS. */
KjarniErrorCode kjarni_hip_answer_plan(const uint32_t* ids, const int32_t* offsets, int32_t n, int32_t head_dim, int32_t min_shared,
                                       int32_t* chunk_first_seq, int32_t* chunk_rows, int32_t* n_chunks, int32_t* groups,
                                       int32_t group_capacity, int32_t* n_groups, int32_t* vec_blocks, int32_t vec_capacity, int32_t* n_vec,
                                       int32_t* mfma_blocks, int32_t mfma_capacity, int32_t* n_mfma, int32_t* prefix_blocks,
                                       int32_t prefix_capacity, int32_t* n_prefix, int32_t* gather, int32_t gather_capacity, int32_t* n_gather);
/* The answer-logits kernel alone, host pointers: out[j, t] = dot(norm(x[src[j], 0 .. hidden)), head[targets[t], :]) for j < n,
 * t < n_targets, out [n, n_targets].  x [x_rows, ldx] f32; head [head_rows, hidden] f32, or bf16 when head_is_bf16.  beta NULL:
 * (x / sqrt(mean(x^2) + eps)) * gamma; beta given: LayerNorm.  hidden 1 .. 16384.  The kernel reads rows src[j] of x, gamma, beta
 * and the targeted head rows, nothing else.  src[j] outside [0, x_rows), targets[t] >= head_rows, n_targets outside 1 ..
 * KJARNI_HIP_ANSWER_MAX_TARGETS: INVALID_CONFIG. */
KjarniErrorCode kjarni_hip_op_answer_logits(int32_t device, const float* x, int64_t ldx, int32_t x_rows, const int32_t* src, int32_t n,
                                            int32_t hidden, const float* gamma, const float* beta, float eps, const void* head,
                                            int32_t head_rows, int32_t head_is_bf16, const uint32_t* targets, int32_t n_targets, float* out);
/* The prompt rule of the decoder rerankers alone (host only), on the tokenizer.json at tokenizer_json_path:
 *   P    = "<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. Note
 *          that the answer can only be \"yes\" or \"no\".<|im_end|>\n<|im_start|>user\n"
 *   body = "<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {document}"
 *   S    = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
 * each encoded on its own (added tokens recognised, no BOS / EOS added); ids = P + body[0 .. max_tokens - |P| - |S|) + S, the body
 * cut from the right so that only the document loses tokens.  instruction NULL: "Given a web search query, retrieve relevant
 * passages that answer the query".  Writes min(n, capacity) ids to ids_out (may be NULL with capacity 0) and n to n_out.
 * INVALID_CONFIG when the cut would reach into the query; LOAD_FAILED when the file does not load, or when "yes" or "no" is not
 * exactly one token of it (the message names the word). */
KjarniErrorCode kjarni_hip_rerank_prompt_ids(const char* tokenizer_json_path, const char* instruction, const char* query, const char* document,
                                             int32_t max_tokens, uint32_t* ids_out, size_t capacity, size_t* n_out);
/* A test hook: kjarni_hip_decoder_answer_rows of a decoder reranker's model (zeros on NULL and on a cross-encoder reranker), so
 * that a test of the string-level calls can see that the query was computed once. */
void kjarni_hip_reranker_answer_rows(const KjarniReranker* reranker, uint64_t* computed, uint64_t* saved);
/* The switch and the counters on the Chat and Generator handles' models (send, generate, score and generate_batch take it). */
KjarniErrorCode kjarni_hip_chat_set_prefix_reuse(KjarniChat* chat, int32_t on);
void kjarni_hip_chat_prefix_stats(KjarniChat* chat, uint64_t* reused, uint64_t* computed);
KjarniErrorCode kjarni_hip_generator_set_prefix_reuse(KjarniGenerator* generator, int32_t on);
/* kjarni_hip_decoder_set_fp8_matrix_cores on the handle's model. */
KjarniErrorCode kjarni_hip_chat_set_fp8_matrix_cores(KjarniChat* chat, int32_t on);
KjarniErrorCode kjarni_hip_generator_set_fp8_matrix_cores(KjarniGenerator* generator, int32_t on);
void kjarni_hip_generator_prefix_stats(KjarniGenerator* generator, uint64_t* reused, uint64_t* computed);

/* ---- device memory helpers for callers without a HIP runtime binding --------- */
KjarniErrorCode kjarni_hip_malloc(int32_t device, size_t bytes, void** out_dev);
KjarniErrorCode kjarni_hip_free(int32_t device, void* ptr_dev);
KjarniErrorCode kjarni_hip_memcpy_h2d(int32_t device, void* dst_dev, const void* src, size_t bytes);
KjarniErrorCode kjarni_hip_memcpy_d2h(int32_t device, void* dst, const void* src_dev, size_t bytes);
KjarniErrorCode kjarni_hip_synchronize(int32_t device);

/* ---- chat, one stage at a time (host side; parity tests) ---------------------------------------
 * Byte-level BPE tokenizer: the `tokenizers` 0.22.1 pipeline for Llama 3 / Qwen 2 / GPT-2 style tokenizer.json
 * (added-token extraction, NFC, Split + ByteLevel, BPE with merge ranks and ignore_merges), as the reference calls
 * it: encode(text, add_special_tokens = false) (crates/kjarni-transformers/src/decoder/generator.rs:141-146),
 * right-truncated to max_length when non-zero (pipeline/decoder/loader.rs:115-120), decode(ids, skip_special). */
typedef struct KjarniBpeTokenizer KjarniBpeTokenizer;
KjarniErrorCode kjarni_bpe_tokenizer_load(const char* tokenizer_json_path, KjarniBpeTokenizer** out);
void kjarni_bpe_tokenizer_free(KjarniBpeTokenizer* tokenizer);
KjarniErrorCode kjarni_bpe_tokenizer_encode(const KjarniBpeTokenizer* tokenizer, const char* text, size_t max_length, uint32_t* ids_out,
                                            size_t capacity, size_t* n_out);
KjarniErrorCode kjarni_bpe_tokenizer_decode(const KjarniBpeTokenizer* tokenizer, const uint32_t* ids, size_t n, int32_t skip_special,
                                            char** out);
KjarniErrorCode kjarni_bpe_tokenizer_pre_tokenize(const KjarniBpeTokenizer* tokenizer, const char* text, KjarniStringArray* out);
/* The embedding entry of the BPE tokenizer: encode(text, add_special_tokens = true).  The `single` template of a
 * TemplateProcessing post-processor (top-level or inside a Sequence) frames the ids: the special tokens before and after $A are
 * added; no post-processor, or ByteLevel alone, adds nothing.  max_length (0: none) truncates the sequence's own tokens from the
 * right so that the framed length is at most max_length; the framing tokens always survive.  A tokenizer.json with any other
 * post-processor type: INVALID_CONFIG naming the type. */
KjarniErrorCode kjarni_bpe_tokenizer_encode_embedding(const KjarniBpeTokenizer* tokenizer, const char* text, size_t max_length,
                                                      uint32_t* ids_out, size_t capacity, size_t* n_out);

/* ChatTemplate::apply (crates/kjarni-transformers/src/chat/{llama3,chatml,mistral}.rs): template_kind 0 = Llama 3
 * (for_generation), 1 = ChatML, 2 = Mistral; roles 0 system / 1 user / 2 assistant. */
KjarniErrorCode kjarni_chat_template_apply(int32_t template_kind, const int32_t* roles, const char* const* contents, size_t n, char** out);

/* sample_token's distribution (crates/kjarni-transformers/src/common/sampling.rs:89-108): top-k, top-p, min-p
 * (negative = not set), temperature, softmax; probs_out[vocab] holds 0 for filtered tokens.  kjarni_sample_from_probs
 * is sample_from_probs (:173-184) for a given draw; kjarni_logits_process applies the repetition penalty (:8-27) and
 * the no-repeat-n-gram ban (:29-57, 0 = off) in place. */
KjarniErrorCode kjarni_sampling_distribution(const float* logits, size_t vocab, float temperature, int64_t top_k, float top_p, float min_p,
                                             float* probs_out);
/* The same distribution decided from CANDIDATES only -- every token whose logit is within `tau` of the maximum, the
 * maximum, and the sum of exp(logit - max) over the vocabulary in a non-index order -- which is what the decode loop's
 * device kernels hand to the host per sampled token instead of 4 x vocab bytes of logits.  *decided = 0 when the
 * candidates do not decide it (a filter reaches past them, or a top-p crossing lies within the rounding of the sum):
 * the loop then fetches the logits and runs kjarni_sampling_distribution's path.  Host-side emulation for parity tests. */
KjarniErrorCode kjarni_sampling_distribution_candidates(const float* logits, size_t vocab, float tau, float temperature, int64_t top_k,
                                                        float top_p, float min_p, float* probs_out, int32_t* decided,
                                                        size_t* n_candidates);
/* The same decision from a candidate list as the device hands it over (no GPU, no emulation): ids / vals [n] in any order,
 * the header's mx, floor and sum.  An id >= vocab: INVALID_CONFIG. */
KjarniErrorCode kjarni_sampling_distribution_from_candidates(const uint32_t* ids, const float* vals, size_t n, float mx, float floor, float sum,
                                                             size_t vocab, float temperature, int64_t top_k, float top_p, float min_p,
                                                             float* probs_out, int32_t* decided);
uint32_t kjarni_sample_from_probs(const float* probs, size_t vocab, float uniform);
KjarniErrorCode kjarni_logits_process(float* logits, size_t vocab, const uint32_t* tokens, size_t n_tokens, float repetition_penalty,
                                      size_t no_repeat_ngram);

/* resolve_generation_config (crates/kjarni/src/generation/resolution.rs:8-85) over the model defaults
 * (llama/model.rs:373-396, qwen/model.rs:261-282, or generation_config_json when it deserializes as
 * HFGenerationDefaults) and the chat mode (mode < 0: no mode defaults, the bare Generator). */
typedef struct KjarniResolvedGeneration {
    int32_t strategy;          /* 0 greedy, 1 sample, 2 beam search */
    float temperature;
    int64_t top_k;             /* -1 = None */
    float top_p;               /* < 0 = None */
    float min_p;               /* < 0 = None */
    float repetition_penalty;
    size_t no_repeat_ngram_size;
    int64_t max_new_tokens;    /* -1 = None */
    size_t max_length;
    int32_t add_bos_token;
} KjarniResolvedGeneration;
KjarniErrorCode kjarni_generation_resolve(const char* model_type, size_t max_position_embeddings, const char* generation_config_json,
                                          int32_t mode, const KjarniGenerationConfig* runtime, KjarniResolvedGeneration* out);

/* On a live chat handle: the resolved config of a call, the prompt the template produces (roles == NULL and n == 0:
 * Chat::create_conversation; otherwise Chat::history_to_conversation; message appended as the user turn when non-NULL),
 * the token ids DecoderGenerator::encode produces for a prompt (BOS rule included), and the seed of the sampler's
 * generator (the reference draws from rand::thread_rng()). */
KjarniErrorCode kjarni_hip_chat_resolve(const KjarniChat* chat, const KjarniGenerationConfig* runtime, KjarniResolvedGeneration* out);
KjarniErrorCode kjarni_hip_chat_format_prompt(const KjarniChat* chat, const int32_t* roles, const char* const* contents, size_t n,
                                              const char* message, char** out);
KjarniErrorCode kjarni_hip_chat_encode(const KjarniChat* chat, const char* prompt, const KjarniGenerationConfig* runtime, uint32_t* ids_out,
                                       size_t capacity, size_t* n_out);
void kjarni_hip_chat_seed(KjarniChat* chat, uint64_t seed);
/* Sampled tokens and the logits processors: by default everything that is O(vocab) runs on the device and the host
 * decides on a candidate list (a 32-byte header + a few hundred (token, logit) pairs per token); 0 = the logits travel
 * to the host for every token, which is the checker the tests compare with -- same tokens for the same seed.  The
 * counters: tokens decided from candidates / tokens that needed the logits after all. */
void kjarni_hip_chat_set_device_sampling(KjarniChat* chat, int32_t on);
void kjarni_hip_chat_sampling_counters(KjarniChat* chat, uint64_t* from_candidates, uint64_t* from_logits);
/* The same hooks on a Generator handle: the resolved config of a call, DecoderGenerator::encode of a prompt (BOS rule
 * included), the sampler's seed, and device (1) or host (0) sampling / logits processors. */
KjarniErrorCode kjarni_hip_generator_resolve(const KjarniGenerator* generator, const KjarniGenerationConfig* runtime,
                                             KjarniResolvedGeneration* out);
KjarniErrorCode kjarni_hip_generator_encode(const KjarniGenerator* generator, const char* prompt, const KjarniGenerationConfig* runtime,
                                            uint32_t* ids_out, size_t capacity, size_t* n_out);
void kjarni_hip_generator_seed(KjarniGenerator* generator, uint64_t seed);
void kjarni_hip_generator_set_device_sampling(KjarniGenerator* generator, int32_t on);

/* ---- constrained decoding: regex-guided generation with a device token mask (NOT in the reference) ----
 * A regular expression restricts what a generate call may emit: after every token, the bytes of all emitted tokens are a prefix
 * of some string the pattern matches in full; in an accepting state the call's stop ids become legal.
 *
 * The pattern compiles, on the host, to a DFA over bytes.  Syntax: literals (non-ASCII ones match as their UTF-8 bytes), the
 * escapes \\ \. \n \t \r \f \v \" \xHH and escaped metacharacters, \d \w \s (ASCII), `.` (any Unicode scalar except \n),
 * classes [a-z0-9_] and negated classes [^...] over ASCII members, groups ( ) and (?: ), alternation, and the quantifiers
 * * + ? {m} {m,} {m,n} with n <= 255.  `.` and a negated class also match every well-formed non-ASCII UTF-8 scalar.  The match is
 * a full match, with the semantics of Python's re.fullmatch(pattern, text, re.ASCII) compared on text.encode().  Anchors, lazy
 * and possessive quantifiers, back-references, look-around, named groups, inline flags, the negated shorthands, a non-ASCII
 * class member, more than KJARNI_CONSTRAINT_MAX_STATES states (the message gives the count) and an empty language:
 * INVALID_CONFIG, the message naming the construct and its byte offset.
 *
 * The table: trans[states][256] (uint16), state 0 the start state, accepting[states], closed[states] (accepting, no live
 * outgoing byte).  The DFA is minimal and holds no state that cannot reach an accepting one: a transition into such a state is
 * KJARNI_CONSTRAINT_DEAD. */
#define KJARNI_CONSTRAINT_DEAD 0xFFFFu
#define KJARNI_CONSTRAINT_MAX_STATES 4096
#define KJARNI_CONSTRAINT_MAX_STOPS 16
typedef struct KjarniHipRegex KjarniHipRegex;
KjarniErrorCode kjarni_hip_regex_compile(const char* pattern, KjarniHipRegex** out);
void kjarni_hip_regex_free(KjarniHipRegex* regex);
KjarniErrorCode kjarni_hip_regex_dims(const KjarniHipRegex* regex, int32_t* states, uint32_t* start);
/* trans_out [states * 256], accepting_out / closed_out [states]; any may be NULL. */
KjarniErrorCode kjarni_hip_regex_table(const KjarniHipRegex* regex, uint16_t* trans_out, uint8_t* accepting_out, uint8_t* closed_out);
/* *state_out = the state after bytes[n] from `state`, KJARNI_CONSTRAINT_DEAD when the walk dies or `state` is no state. */
KjarniErrorCode kjarni_hip_regex_step(const KjarniHipRegex* regex, uint32_t state, const uint8_t* bytes, size_t n, uint32_t* state_out);
/* The raw bytes token `id` contributes to the output (not through decode, which trims): byte-level BPE: the GPT-2 byte map
 * inverted; the SentencePiece-style shape: U+2581 -> space, <0xNN> -> that byte; added and special tokens, and ids the file does
 * not define: zero bytes.  Writes min(*n_out, capacity) bytes. */
KjarniErrorCode kjarni_bpe_tokenizer_token_bytes(const KjarniBpeTokenizer* tokenizer, uint32_t id, uint8_t* bytes_out, size_t capacity,
                                                 size_t* n_out);
/* The device constraint: the DFA, the token table (token t contributes tok_bytes[tok_off[t], tok_off[t + 1]); tok_off has
 * vocab + 1 entries) and the mask built from them on the device: mask[states][ceil(vocab / 64)] 64-bit words, bit (q, t) set iff
 * token t has at least one byte and walking its bytes from q never reaches DEAD, and count[states], the set bits per state.
 * A mask beyond 256 MiB or a malformed table: INVALID_CONFIG before any GPU work.  The regex may be freed afterwards. */
typedef struct KjarniHipConstraint KjarniHipConstraint;
KjarniErrorCode kjarni_hip_constraint_new(int32_t device, const KjarniHipRegex* regex, const uint32_t* tok_off, const uint8_t* tok_bytes,
                                          int32_t vocab, KjarniHipConstraint** out);
void kjarni_hip_constraint_free(KjarniHipConstraint* constraint);
KjarniErrorCode kjarni_hip_constraint_dims(const KjarniHipConstraint* constraint, int32_t* states, int32_t* vocab, int32_t* words);
KjarniErrorCode kjarni_hip_constraint_mask(const KjarniHipConstraint* constraint, uint32_t state, uint64_t* words_out);
KjarniErrorCode kjarni_hip_constraint_counts(const KjarniHipConstraint* constraint, uint32_t* counts_out);
/* The three kernels alone, through the launchers the loops run, with a guard band behind every output buffer.
 * kjarni_hip_op_constraint_mask: the mask build on tables given by the host: mask_out [states * ceil(vocab / 64)], counts_out
 * [states].
 * kjarni_hip_op_constraint_apply: logits [rows, ld] (ld >= vocab) with the per-row states[rows] and done[rows] flags and the stop
 * ids (n_stop <= 16): where done is clear, a logit keeps its bits when its token's mask bit is set, or, for a stop id, when the
 * state is accepting (whatever the stop id's bytes); every other logit of the row becomes -inf.  logits_out [rows, ld]: all of it,
 * the floats between vocab and ld included.
 * kjarni_hip_op_constraint_advance: picked[rows] moves states[rows] / done[rows] in place and writes violated_out[rows]: a stop
 * id in an accepting state keeps the state and sets done; any other token walks its bytes, done when the new state is closed;
 * a token the mask does not allow sets violated (and done: the state no longer moves).  A row whose done is set is left alone. */
KjarniErrorCode kjarni_hip_op_constraint_mask(int32_t device, const uint16_t* trans, int32_t states, const uint32_t* tok_off,
                                              const uint8_t* tok_bytes, int32_t vocab, uint64_t* mask_out, uint32_t* counts_out);
KjarniErrorCode kjarni_hip_op_constraint_apply(int32_t device, const KjarniHipConstraint* constraint, const float* logits, int32_t rows, int64_t ld,
                                               const uint32_t* states, const int32_t* done, const uint32_t* stop_ids, int32_t n_stop,
                                               float* logits_out);
KjarniErrorCode kjarni_hip_op_constraint_advance(int32_t device, const KjarniHipConstraint* constraint, const int32_t* picked, int32_t rows,
                                                 uint32_t* states, int32_t* done, const uint32_t* stop_ids, int32_t n_stop,
                                                 int32_t* violated_out);
/* How a constrained call ended.  final_state: the automaton's state after the emitted tokens, as the host walked it;
 * device_state: the same as the device left it (the device sampling route and plain greedy; equal to final_state unless violated);
 * accepted: final_state is accepting; complete: the run ended on a stop id in an accepting state or in a closed state (not on a
 * limit or the callback); violated: a token outside the mask was picked (never, unless the logits are all NaN). */
typedef struct KjarniHipConstraintResult { uint32_t final_state, device_state; int32_t accepted, complete, violated; } KjarniHipConstraintResult;
/* kjarni_hip_decoder_generate_sampled's plain loop (no lookup, no drafter) under a constraint.  Every step applies the mask
 * before any logits processor and before the pick or the cut: plain greedy replays a captured chain pass -> apply -> argmax ->
 * advance in bursts; with processors or sampling the order is apply, processors, argmax or the sampler's cut, and the state
 * advances after the token is fed; with device sampling off the same mask is applied to the host copy of the logits.  Reaching a
 * closed state ends the run without a stop token.  Before any GPU work, INVALID_CONFIG: a constraint of another device or
 * vocabulary, more than 16 stop ids, and a state a run can be in (the start state and what the allowed tokens lead to from it)
 * that is neither closed, nor accepting with stop ids in the call, nor offers a token that is no stop id (the message names the
 * state).  result may be NULL. */
KjarniErrorCode kjarni_hip_decoder_generate_constrained(KjarniHipDecoder* decoder, const KjarniHipConstraint* constraint, const uint32_t* prompt,
                                                        size_t n_prompt, const KjarniHipSamplingOptions* options, KjarniTokenCallbackFn on_token,
                                                        void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out,
                                                        KjarniHipConstraintResult* result);
/* A pattern for every later request of the handle (NULL or "": none, the plain behaviour).  The token table comes from the
 * handle's own tokenizer, built once per pattern; the compiled constraint is kept until the pattern changes.  While set, requests
 * run through the plain loop even when prompt lookup or a draft model is switched on; generate_batch constrains every prompt of the batch on its lane
 * (kjarni_hip_generator_batch_constraint_result). */
KjarniErrorCode kjarni_hip_generator_set_constraint(KjarniGenerator* generator, const char* pattern);
KjarniErrorCode kjarni_hip_chat_set_constraint(KjarniChat* chat, const char* pattern);
/* The result of the handle's last constrained request (zeros before one). */
KjarniErrorCode kjarni_hip_generator_constraint_result(const KjarniGenerator* generator, KjarniHipConstraintResult* out);
KjarniErrorCode kjarni_hip_chat_constraint_result(const KjarniChat* chat, KjarniHipConstraintResult* out);

/* ---- constrained decoding with a stack: grammars compiled to a stack automaton, and its two kernels (NOT in the reference) ----
 * A grammar is a list of rules (name, pattern); rule 0 is the start rule.  A pattern is the syntax above plus one construct,
 * (?&name): a string of rule `name` here (names are [A-Za-z_][A-Za-z0-9_]*; kjarni_hip_regex_compile keeps refusing the
 * construct).  The language is the context-free language the rules define, full match from rule 0, over bytes, with at most
 * KJARNI_GRAMMAR_MAX_DEPTH calls open at a time: a string that nests deeper is not matched.
 *
 * Each rule compiles to a DFA over bytes and one symbol per called rule; the states of all rules share one numbering, state 0
 * the start state of rule 0.  The table: action[states][256] (uint32) and flags[states].  Entry bits 31..30: 0 none, 1 move,
 * 2 call.  A move holds the next state in bits 11..0; a call holds the callee's start state in bits 11..0 and the state to return
 * to in bits 23..12.  Flags bit 0: accepting in its rule; bit 1: no_out, no byte has a move or a call.  One byte b at (state q,
 * stack of return states, depth d):
 *     loop: a = action[q][b]
 *           move: q = a.next; done
 *           call: d == 64 -> dead;  push a.ret;  q = a.next;  again      (the callee sees the same byte)
 *           none: accepting[q] and d > 0 -> q = pop;  again               (the rule ended before this byte)
 *                 otherwise dead
 * A configuration is accepted when every level (the state and all return states) is accepting, and closed when every level is
 * no_out.  The machine is deterministic by construction, and the compiler refuses, INVALID_CONFIG with the rule named (and the
 * byte, where there is one), every grammar for which it would not recognise exactly the grammar's language: two ways to continue
 * on one byte in one state (a byte edge and the FIRST set of a call, or two calls); a rule that may either end or go on at a byte
 * that may also follow one of its calls (LL(1): FOLLOW through accepting return states, transitively); a called rule that matches
 * the empty string; left recursion, direct or through a chain of first calls; a rule with no finite string; an undefined, duplicate
 * or bad name; more than KJARNI_GRAMMAR_MAX_RULES rules or KJARNI_GRAMMAR_MAX_STATES states (the message gives the count); and
 * every per-pattern refusal above, prefixed with the rule's name.  Rules that rule 0 never reaches are dropped. */
#define KJARNI_GRAMMAR_MAX_RULES 256
#define KJARNI_GRAMMAR_MAX_STATES 4096
#define KJARNI_GRAMMAR_MAX_DEPTH 64
#define KJARNI_GRAMMAR_TOKEN_PUSHES 16
typedef struct KjarniHipGrammar KjarniHipGrammar;
KjarniErrorCode kjarni_hip_grammar_compile(const char* const* names, const char* const* patterns, int32_t n_rules, KjarniHipGrammar** out);
void kjarni_hip_grammar_free(KjarniHipGrammar* grammar);
/* rules: the rules kept (those rule 0 reaches). */
KjarniErrorCode kjarni_hip_grammar_dims(const KjarniHipGrammar* grammar, int32_t* states, int32_t* rules);
/* action_out [states * 256], flags_out [states], rule_of_out [states] (the kept rule a state belongs to, rule 0 first); any may
 * be NULL. */
KjarniErrorCode kjarni_hip_grammar_table(const KjarniHipGrammar* grammar, uint32_t* action_out, uint8_t* flags_out, uint16_t* rule_of_out);
/* The walk of bytes[n] from (state, stack[depth], depth), on the host.  *alive_out = 0 when the walk dies or the start is no
 * configuration of the table (the other outputs are then left alone); else state_out, depth_out and stack_out [64, written up to
 * the new depth].  as_token != 0: the bytes are one token's, and a walk that holds more than KJARNI_GRAMMAR_TOKEN_PUSHES of its
 * own pushes at once dies: the rule the kernels keep. */
KjarniErrorCode kjarni_hip_grammar_walk(const KjarniHipGrammar* grammar, uint32_t state, const uint16_t* stack, int32_t depth, const uint8_t* bytes,
                                        size_t n, int32_t as_token, uint32_t* state_out, uint16_t* stack_out, int32_t* depth_out, int32_t* alive_out);
/* The device object: the automaton and a token table (as kjarni_hip_constraint_new takes it) in device memory.  There is no
 * mask made once per state: which tokens are legal depends on the stack.  A malformed table: INVALID_CONFIG before any GPU work.
 * The grammar may be freed afterwards. */
typedef struct KjarniHipGrammarConstraint KjarniHipGrammarConstraint;
KjarniErrorCode kjarni_hip_grammar_constraint_new(int32_t device, const KjarniHipGrammar* grammar, const uint32_t* tok_off, const uint8_t* tok_bytes,
                                                  int32_t vocab, KjarniHipGrammarConstraint** out);
void kjarni_hip_grammar_constraint_free(KjarniHipGrammarConstraint* constraint);
KjarniErrorCode kjarni_hip_grammar_constraint_dims(const KjarniHipGrammarConstraint* constraint, int32_t* states, int32_t* vocab);
/* The two kernels alone, through their launchers, with a guard band behind every output buffer; every refusal (dimensions, a row
 * that is no configuration of the automaton, more than 16 stop ids, another device) is made before any GPU work.  A row is
 * states[r], depths[r] (0..64), stacks[r][64] and done[r].
 * kjarni_hip_op_grammar_apply: logits [rows, ld] (rows <= 64, ld >= vocab): where done is clear, every token's bytes are walked
 * from the row's configuration; a logit keeps its bits when its token has at least one byte and the walk does not die, or, for a
 * stop id, when the configuration is accepted (whatever the stop id's bytes); every other logit of the row becomes -inf.
 * logits_out [rows, ld]: all of it, the floats between vocab and ld included.
 * kjarni_hip_op_grammar_advance: picked[rows] moves the rows in place and writes violated_out[rows]: a stop id in an accepted
 * configuration keeps it and sets done; any other token walks its bytes and moves state, depth and stack (the stack words above the
 * new depth are left as they were), done when the new configuration is closed; a token apply masks sets violated and done and
 * moves nothing.  A row whose done is set is left alone.  log_cap > 0 (rows == 1 only): the state and depth after the step are
 * stored at state_log[log_count - 1] / depth_log[log_count - 1] when that index is within log_cap, as the generation loop logs
 * them behind each recorded pick; both arrays [log_cap], passed in and out. */
KjarniErrorCode kjarni_hip_op_grammar_apply(int32_t device, const KjarniHipGrammarConstraint* constraint, const float* logits, int32_t rows, int64_t ld,
                                            const uint32_t* states, const int32_t* depths, const uint16_t* stacks, const int32_t* done,
                                            const uint32_t* stop_ids, int32_t n_stop, float* logits_out);
KjarniErrorCode kjarni_hip_op_grammar_advance(int32_t device, const KjarniHipGrammarConstraint* constraint, const int32_t* picked, int32_t rows,
                                              uint32_t* states, int32_t* depths, uint16_t* stacks, int32_t* done, const uint32_t* stop_ids,
                                              int32_t n_stop, int32_t* violated_out, int32_t log_count, int32_t log_cap, uint32_t* state_log,
                                              int32_t* depth_log);
/* How a grammar-constrained call ended.  final_state / final_depth: the configuration's state and stack depth after the emitted
 * tokens, as the host walked them; device_state / device_depth: the same as the device left them (equal unless violated);
 * accepted: every level of the final configuration is accepting; complete: the run ended on a stop id in an accepted
 * configuration or in a closed one (not on a limit or the callback); violated: a token outside the mask was picked (all-NaN
 * logits, or a configuration with nothing left that the refusal below let through). */
typedef struct KjarniHipGrammarResult { uint32_t final_state, device_state; int32_t final_depth, device_depth, accepted, complete, violated; } KjarniHipGrammarResult;
/* kjarni_hip_decoder_generate_constrained with a grammar in the constraint's place: the same loop.  Plain greedy replays a third
 * captured chain pass -> grammar apply -> argmax -> grammar advance in bursts, the host walking its own configuration per drained
 * token; with processors or sampling the order is apply, processors, argmax or the sampler's cut, and the device automaton takes
 * the host's choice before the token is fed; with device sampling off the same mask is applied to the host copy of the logits from
 * the host's walk.  The run ends at a stop id, a closed configuration or the limits.  Before any GPU work, INVALID_CONFIG: a
 * grammar constraint of another device or vocabulary, more than 16 stop ids, and the refusal on states: a state a run can be in
 * (state 0 and wherever a token can end from such a state, a walk that pops below the token's own pushes going on in every return
 * state of the calls of the rule it leaves: an over-approximation) that offers no token other than a stop id and is either not
 * accepting, or accepting in rule 0 with a way on while the call has no stop id (the message names the state and its rule).  What
 * that lets through is caught at run time and ends the run with violated = 1.  The lookup and draft entries refuse a grammar as they
 * refuse a constraint; the lanes take one per prompt (kjarni_hip_decoder_generate_wide_constrained).  result may be NULL. */
KjarniErrorCode kjarni_hip_decoder_generate_grammar(KjarniHipDecoder* decoder, const KjarniHipGrammarConstraint* grammar, const uint32_t* prompt,
                                                    size_t n_prompt, const KjarniHipSamplingOptions* options, KjarniTokenCallbackFn on_token,
                                                    void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out,
                                                    KjarniHipGrammarResult* result);
/* A grammar for every later request of the handle, as kjarni_hip_generator_set_constraint sets a pattern (names / patterns NULL or
 * n_rules <= 0: none).  A handle holds a pattern or a grammar: setting a grammar clears a set pattern and the other way round.  The
 * token table comes from the handle's own tokenizer.  A refused grammar leaves the handle as it was. */
KjarniErrorCode kjarni_hip_generator_set_grammar(KjarniGenerator* generator, const char* const* names, const char* const* patterns, int32_t n_rules);
KjarniErrorCode kjarni_hip_chat_set_grammar(KjarniChat* chat, const char* const* names, const char* const* patterns, int32_t n_rules);
/* The result of the handle's last request under a grammar (zeros before one). */
KjarniErrorCode kjarni_hip_generator_grammar_result(const KjarniGenerator* generator, KjarniHipGrammarResult* out);
KjarniErrorCode kjarni_hip_chat_grammar_result(const KjarniChat* chat, KjarniHipGrammarResult* out);

/* ---- generation log-probabilities: per emitted token its logprob and the top_k most likely alternatives ------------------------
 * The distribution is the log-softmax of the logits as the vocabulary head wrote them: before the constraint or grammar mask,
 * before the repetition penalty and the n-gram ban, before temperature and the sampler's cut -- kjarni_hip_decoder_score's
 * distribution, so generating and then scoring prompt + output gives the same numbers inside the float bar.  The top_k
 * alternatives are in kjarni_hip_decoder_score_topk's order: descending logit, among equal logits the larger id first; slot 0 is
 * the greedy pick of the unmasked row.  top_k is 0 .. KJARNI_SCORE_TOPK_MAX and not above the vocabulary; 0 gives the emitted
 * token's logprob alone.
 *
 * The slab rule of the kernels (0 outside rows 1..64 / vocab >= 1): slabs = min(64, ceil(vocab / 1024), max(1, ceil(512 / rows))),
 * the slab length rounded up to a multiple of 4 elements and the slabs recounted over it.  No device is touched. */
int32_t kjarni_hip_token_logprob_slabs(int32_t rows, int32_t vocab);
/* The kernel pair alone on logits given by the host: one launch pair per call over logits [calls, rows, ld] (rows 1..64,
 * ld >= vocab; what lies behind `vocab` in a row is not read).  tokens [calls, rows]: the chosen token of each row, -1 = skip:
 * the outputs of a skipped row come back as the caller passed them.  logprob_out / lse_out [calls, rows], topk_ids_out /
 * topk_logprob_out [calls, rows, top_k]; every output but logprob_out may be NULL.  *slabs_out: the slabs a row was cut into.
 * Odd calls take the raw copy in the slab pass and read the chosen logit from it (INFERENCE_FAILED when the copy is not the
 * row, or a guard band behind a device buffer was touched).  Every argument is checked before a device is asked for:
 * INVALID_CONFIG names it. */
KjarniErrorCode kjarni_hip_op_token_logprobs(int32_t device, const float* logits, int32_t calls, int32_t rows, int64_t ld, int32_t vocab,
                                             const int32_t* tokens, int32_t top_k, float* logprob_out, uint32_t* topk_ids_out,
                                             float* topk_logprob_out, float* lse_out, int32_t* slabs_out);
/* Timing for tools/bench_more.py: the milliseconds of one launch pair over logits [rows, vocab] (rows 1..64, top_k 1..8) and of
 * the one-workgroup-per-row score kernel (the rows route of kjarni_hip_decoder_score_topk, 8 rows a launch) over the same rows,
 * each the mean of `iters` back-to-back repeats between two events. */
KjarniErrorCode kjarni_hip_op_token_logprobs_bench(int32_t device, const float* logits, int32_t rows, int32_t vocab, int32_t top_k, int32_t iters,
                                                   float* pair_ms_out, float* score_rows_ms_out);
/* The plain loop of kjarni_hip_decoder_generate_sampled (no lookup, no drafter: a request that asks for log-probabilities takes
 * the plain loop), under `constraint` or `grammar` when one is given (both: INVALID_CONFIG), with the records of the first
 * min(*n_out, capacity) emitted tokens: logprob_out [capacity], topk_ids_out / topk_logprob_out [capacity, top_k] (NULL allowed
 * for each; entries past the emitted tokens are not written).  The ids are those of the entry without log-probabilities for
 * the same options and draws.  A stop id is not emitted and has no record.  Plain greedy replays a chain of its own, pass ->
 * slab pass -> argmax -> record (constrained: pass -> slab pass with the raw copy -> apply -> argmax -> record -> advance),
 * the records fetched with the tokens; with processors or sampling the slab pass runs ahead of the mask and the processors and
 * the record is written once the host has decided; with device sampling off the host computes the record in float32 from the
 * raw row.  Refusals are those entries', plus top_k outside 0 .. KJARNI_SCORE_TOPK_MAX or above the vocabulary
 * (INVALID_CONFIG naming top_k), before any GPU work, with the outputs and the cache untouched.  constraint_result /
 * grammar_result may be NULL. */
KjarniErrorCode kjarni_hip_decoder_generate_logprobs(KjarniHipDecoder* decoder, const KjarniHipConstraint* constraint,
                                                     const KjarniHipGrammarConstraint* grammar, const uint32_t* prompt, size_t n_prompt,
                                                     const KjarniHipSamplingOptions* options, int32_t top_k, KjarniTokenCallbackFn on_token,
                                                     void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out, float* logprob_out,
                                                     uint32_t* topk_ids_out, float* topk_logprob_out, KjarniHipConstraintResult* constraint_result,
                                                     KjarniHipGrammarResult* grammar_result);
/* kjarni_hip_decoder_generate_wide with records: its arguments, then top_k and logprob_out [n, capacity], topk_ids_out /
 * topk_logprob_out [n, capacity, top_k] (NULL allowed for each), prompt i's records for its first min(n_out[i], capacity) tokens.
 * Every width 1..64 is served (8 or fewer on the lanes step, as kjarni_hip_decoder_generate_wide forwards).  The kernel pair
 * runs over all lane rows in one launch ahead of the pick, inside the captured step; a lane's record index is its own
 * device-held count, so a lane that takes the next waiting prompt starts at record 0.  A request with a penalty or an n-gram
 * ban is recorded lane by lane, as the single-sequence loop does.  The ids are kjarni_hip_decoder_generate_wide's.  top_k outside
 * 0 .. KJARNI_SCORE_TOPK_MAX or above the vocabulary: INVALID_CONFIG naming top_k, before any GPU work. */
KjarniErrorCode kjarni_hip_decoder_generate_wide_logprobs(KjarniHipDecoder* decoder, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                          const size_t* max_new_tokens, float repetition_penalty, int32_t no_repeat_ngram_size,
                                                          int32_t lanes, int32_t lane_context, KjarniBatchTokenCallbackFn on_token,
                                                          void* user_data, uint32_t* ids_out, size_t capacity, size_t* n_out, int32_t top_k,
                                                          float* logprob_out, uint32_t* topk_ids_out, float* topk_logprob_out);
/* Log-probabilities for every later request of the handle: top_k 0 .. KJARNI_SCORE_TOPK_MAX (not above the vocabulary), -1 = off
 * (the default); another value is INVALID_CONFIG and leaves the handle as it was.  While set, generate / stream / send take the
 * plain loop even when prompt lookup or a draft model is switched on, as under a constraint, and generate_batch records every
 * prompt on its lanes. */
KjarniErrorCode kjarni_hip_generator_set_logprobs(KjarniGenerator* generator, int32_t top_k);
KjarniErrorCode kjarni_hip_chat_set_logprobs(KjarniChat* chat, int32_t top_k);
/* The tokens the handle's last generate / stream / send* call emitted (prompt_index 0) -- or prompt `prompt_index` of its last
 * generate_batch call -- with their log-probabilities and alternatives, as kjarni_generator_score_tokens lays them out.  Zeros
 * before any call, after a call that ran with log-probabilities off, and for an index the call did not have.  Free with
 * kjarni_token_scores_free. */
KjarniErrorCode kjarni_hip_generator_last_logprobs(const KjarniGenerator* generator, size_t prompt_index, KjarniTokenScores* out);
KjarniErrorCode kjarni_hip_chat_last_logprobs(const KjarniChat* chat, KjarniTokenScores* out);

/* ---- constrained decoding in the lanes: a pattern or a grammar per prompt, up to 64 prompts in lock step ----------------------
 * The device keeps one table of KJARNI_HIP_WIDE_LANES slots for both lane sets; slot l holds the kind of the request in lane l
 * (0 none, 1 pattern, 2 grammar), that request's tables and stop ids, and the lane's row (pattern: state, done, violated; grammar:
 * state, depth, done, violated, stack[64]).  Two kernels read it:
 *   lane apply    grid (ceil(vocab / 256), lanes): the mask of kjarni_hip_op_constraint_apply or the walk of
 *                 kjarni_hip_op_grammar_apply from the lane's own slot, by the same rules (an allowed logit keeps its bits, a stop id
 *                 is governed by accepting / accepted alone, everything else becomes -inf); nothing is written for a frozen lane
 *                 (live == 0), a lane of kind 0 or a done row.  The logits are rewritten in place and the lanes' pick runs on them.
 *   lane advance  one thread per lane, right behind the lanes' pick: for a lane that was live at the pick, the picked token (the
 *                 lane's newest history entry) moves the lane's row as kjarni_hip_op_constraint_advance / _grammar_advance would.
 *                 A stop id in an accepting state (accepted configuration) sets done; a closed state (configuration) sets done and
 *                 clears live -- the token stays in the history, nothing more is fed; a token the mask would not have allowed sets
 *                 violated and done and clears live.  The limit, the full cache and the token hand-over stay the pick's.
 * The two test hooks below make ONE launcher call on host arrays, check every argument before a device is asked for
 * (INVALID_CONFIG names it), keep a guard band behind every device buffer and return their outputs whole.  Per lane l of
 * [first_lane, first_lane + lanes): kinds[l] and, by kind, constraints[l] or grammars[l] (the other may be NULL; both arrays
 * [64], as every per-lane array here), states[l], depths[l], stacks[l][64], done[l], and the lane's stop ids stop_ids[l][16] /
 * n_stop[l] (the automaton's own: independent of state->stop).  Lanes outside the range are neither read nor written. */
/* KjarniHipWideState for the 8-lane set (kjarni_hip_decoder_generate_batch's lanes): the same fields, 8 entries each. */
#define KJARNI_HIP_BATCH_LANES 8
typedef struct KjarniHipLaneState {
    int32_t token[KJARNI_HIP_BATCH_LANES];
    int32_t pos[KJARNI_HIP_BATCH_LANES];
    int32_t live[KJARNI_HIP_BATCH_LANES];
    int32_t count[KJARNI_HIP_BATCH_LANES];
    int32_t limit[KJARNI_HIP_BATCH_LANES];
    int32_t n_stop[KJARNI_HIP_BATCH_LANES];
    int32_t stop[KJARNI_HIP_BATCH_LANES][KJARNI_HIP_LANE_STOPS];
} KjarniHipLaneState;
/* logits [first_lane + lanes, ld] -> logits_out (the same shape, all of it). */
KjarniErrorCode kjarni_hip_op_lane_automaton_apply(int32_t device, const float* logits, int64_t ld, int32_t vocab, int32_t lanes, int32_t first_lane,
                                                   const int32_t* live, const int32_t* kinds, const KjarniHipConstraint* const* constraints,
                                                   const KjarniHipGrammarConstraint* const* grammars, const uint32_t* states, const int32_t* depths,
                                                   const uint16_t* stacks, const int32_t* done, const uint32_t* stop_ids, const int32_t* n_stop,
                                                   float* logits_out);
/* kjarni_hip_op_wide_pick (wide != 0: state is a KjarniHipWideState, history [64, hist_stride]; wide == 0: the 8-lane layout, the
 * same fields with 8 entries each and stop [8][16], history [8, hist_stride], lanes within 0..8) followed by the lane advance:
 * state and history are picked in place, states / depths / stacks / done move in place, violated_out [64] is written for the
 * lanes of the range. */
KjarniErrorCode kjarni_hip_op_lane_automaton_pick(int32_t device, int32_t wide, const float* logits, int64_t ld, int32_t vocab, int32_t lanes,
                                                  int32_t first_lane, void* state, int32_t* history, int32_t hist_stride, int32_t capacity,
                                                  int32_t advance, const int32_t* kinds, const KjarniHipConstraint* const* constraints,
                                                  const KjarniHipGrammarConstraint* const* grammars, uint32_t* states, int32_t* depths,
                                                  uint16_t* stacks, int32_t* done, const uint32_t* stop_ids, const int32_t* n_stop,
                                                  int32_t* violated_out);
/* How prompt i of a constrained lane call ended: kind (0 none, 1 pattern, 2 grammar) and the fields of KjarniHipGrammarResult
 * (depths 0 under a pattern).  device_state / device_depth: the lane's row as read back when the lane went dead on the device;
 * the host's values where the callback ended the prompt. */
typedef struct KjarniHipLaneAutomatonResult {
    int32_t kind;
    uint32_t final_state, device_state;
    int32_t final_depth, device_depth, accepted, complete, violated;
} KjarniHipLaneAutomatonResult;
/* kjarni_hip_decoder_generate_wide_logprobs with an automaton per prompt: its arguments (top_k = -1: no records), then
 * constraints [n] and grammars [n] (either array may be NULL, and so may any entry: a prompt with neither runs as in
 * kjarni_hip_decoder_generate_wide) and results [n] (may be NULL).  A lane that takes prompt i gets that prompt's tables, the
 * model's stop ids and a fresh row before its first pick; greedy prompts replay one captured chain step -> (slab pass) -> lane
 * apply -> pick -> lane advance (-> record) per (lane set, width, records), prompts with a penalty or an n-gram ban are decided
 * lane by lane with the mask ahead of the processors.  Prompt i's ids and result are those of
 * kjarni_hip_decoder_generate_constrained / _grammar / _generate on that prompt alone; the records stay those of the raw
 * distribution.  Widths of 8 or fewer run the 8-lane set.  Before any GPU work, INVALID_CONFIG naming the prompt index: both a
 * constraint and a grammar for one prompt, an automaton of another device or vocabulary, more than 16 stop ids, and the refusal
 * on states of that prompt's automaton; the other refusals are kjarni_hip_decoder_generate_wide_logprobs'.  The lookup and draft
 * entries keep refusing constraints. */
KjarniErrorCode kjarni_hip_decoder_generate_wide_constrained(KjarniHipDecoder* decoder, const uint32_t* prompt_ids, const size_t* offsets, size_t n,
                                                             const size_t* max_new_tokens, float repetition_penalty,
                                                             int32_t no_repeat_ngram_size, int32_t lanes, int32_t lane_context,
                                                             KjarniBatchTokenCallbackFn on_token, void* user_data, uint32_t* ids_out,
                                                             size_t capacity, size_t* n_out, int32_t top_k, float* logprob_out,
                                                             uint32_t* topk_ids_out, float* topk_logprob_out,
                                                             const KjarniHipConstraint* const* constraints,
                                                             const KjarniHipGrammarConstraint* const* grammars,
                                                             KjarniHipLaneAutomatonResult* results);
/* generate_batch under the handle's pattern or grammar: every prompt of the batch is constrained by it on its lane, and this is
 * the result of prompt `prompt_index` of the handle's last generate_batch call (zeros, kind 0, before one, after an
 * unconstrained one and for an index the call did not have). */
KjarniErrorCode kjarni_hip_generator_batch_constraint_result(const KjarniGenerator* generator, size_t prompt_index,
                                                             KjarniHipLaneAutomatonResult* out);
/* Test hook: the seed of the generator that prompt `prompt_index` of the handle's last generate_batch call drew from (every prompt
 * of a batch draws from its own, seeded from the handle's in prompt order at call start); 1 for a greedy batch, 0 for NULL or an index
 * the call did not have.  kjarni_hip_generator_seed with it, then generate of that prompt alone, takes the same draws. */
uint64_t kjarni_hip_generator_batch_seed(const KjarniGenerator* generator, size_t prompt_index);

#ifdef __cplusplus
}
#endif

#endif /* KJARNI_HIP_H */
