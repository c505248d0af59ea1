// C ABI of constrained decoding (kjarni_hip.h): the pattern compiler (host only), the device constraint, and the three kernels
// alone on tables and logits given by the host.  Error conventions as ffi_llm.cpp: NULL arguments are NULL_POINTER, everything
// else goes through guarded().
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kjarni_hip.h"
#include "ffi_common.h"
#include "ffi_constraint.h"
#include "host_util.h"

using namespace kjarni;

static_assert(KJARNI_CONSTRAINT_DEAD == kConstraintDead, "header constant");
static_assert(KJARNI_CONSTRAINT_MAX_STATES == kConstraintMaxStates, "header constant");
static_assert(KJARNI_CONSTRAINT_MAX_STOPS == kConstraintMaxStops, "header constant");

namespace {

struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { hip_check(hipMalloc(&p, bytes ? bytes : 4), "hipMalloc"); }
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// An output buffer with a guard band behind it (hip_api.cpp's GuardedBuf): check() throws when a kernel wrote past the end.
struct Guarded {
    static constexpr uint32_t kGuard = 0x7fc0beefu;
    static constexpr size_t kGuardWords = 64;
    size_t bytes;
    DevBuf buf;
    explicit Guarded(size_t b) : bytes((b + 7) / 8 * 8), buf(bytes + kGuardWords * 4)
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

void use_device(int32_t device)
{
    const int n = visible_device_count();
    if (n <= 0) throw GpuUnavailable("no HIP device is visible");
    if (device < 0 || device >= n) throw GpuUnavailable("HIP device index out of range");
    hip_check(hipSetDevice(device), "hipSetDevice");
}

void check_table(const uint32_t* tok_off, int32_t vocab)
{
    if (vocab < 1) throw InvalidConfig("vocab must be at least 1");
    if (tok_off[0] != 0) throw InvalidConfig("tok_off[0] must be 0");
    for (int32_t t = 0; t < vocab; ++t)
        if (tok_off[t + 1] < tok_off[t]) throw InvalidConfig("tok_off decreases at token " + std::to_string(t));
}

std::vector<uint32_t> stop_list(const uint32_t* stop_ids, int32_t n_stop)
{
    if (n_stop < 0 || n_stop > kConstraintMaxStops)
        throw InvalidConfig("n_stop must be 0.." + std::to_string(kConstraintMaxStops) + ", got " + std::to_string(n_stop));
    return std::vector<uint32_t>(stop_ids, stop_ids + n_stop);
}

}  // namespace

// ---- the compiler (no GPU) -------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_regex_compile(const char* pattern, KjarniHipRegex** out)
{
    if (!pattern || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_INVALID_CONFIG, [&] {
        auto h = std::make_unique<KjarniHipRegex>();
        try {
            h->dfa = compile_constraint(pattern);
        } catch (const ConstraintError& e) {
            throw InvalidConfig(e.what());
        }
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_regex_free(KjarniHipRegex* regex) { delete regex; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_regex_dims(const KjarniHipRegex* regex, int32_t* states, uint32_t* start)
{
    if (!regex) return KJARNI_ERROR_NULL_POINTER;
    if (states) *states = regex->dfa.states();
    if (start) *start = regex->dfa.start;
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_regex_table(const KjarniHipRegex* regex, uint16_t* trans_out, uint8_t* accepting_out, uint8_t* closed_out)
{
    if (!regex) return KJARNI_ERROR_NULL_POINTER;
    const ConstraintDfa& d = regex->dfa;
    if (trans_out) std::memcpy(trans_out, d.trans.data(), d.trans.size() * sizeof(uint16_t));
    if (accepting_out) std::memcpy(accepting_out, d.accepting.data(), d.accepting.size());
    if (closed_out) std::memcpy(closed_out, d.closed.data(), d.closed.size());
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_regex_step(const KjarniHipRegex* regex, uint32_t state, const uint8_t* bytes, size_t n, uint32_t* state_out)
{
    if (!regex || !state_out || (n && !bytes)) return KJARNI_ERROR_NULL_POINTER;
    *state_out = regex->dfa.step(state, bytes, n);
    return KJARNI_OK;
}

// ---- the device constraint -------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_constraint_new(int32_t device, const KjarniHipRegex* regex, const uint32_t* tok_off,
                                                        const uint8_t* tok_bytes, int32_t vocab, KjarniHipConstraint** out)
{
    if (!regex || !tok_off || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        check_table(tok_off, vocab);
        if (tok_off[vocab] && !tok_bytes) throw InvalidConfig("tok_bytes is NULL but tok_off names " + std::to_string(tok_off[vocab]) + " bytes");
        TokenTable table;
        table.off.assign(tok_off, tok_off + vocab + 1);
        if (tok_off[vocab]) table.bytes.assign(tok_bytes, tok_bytes + tok_off[vocab]);
        auto h = std::make_unique<KjarniHipConstraint>();
        h->inner = std::make_unique<DeviceConstraint>(device, regex->dfa, std::move(table));
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_constraint_free(KjarniHipConstraint* constraint) { delete constraint; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_constraint_dims(const KjarniHipConstraint* constraint, int32_t* states, int32_t* vocab, int32_t* words)
{
    if (!constraint) return KJARNI_ERROR_NULL_POINTER;
    if (states) *states = constraint->inner->dfa().states();
    if (vocab) *vocab = constraint->inner->vocab();
    if (words) *words = constraint->inner->words();
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_constraint_mask(const KjarniHipConstraint* constraint, uint32_t state, uint64_t* words_out)
{
    if (!constraint || !words_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] { constraint->inner->mask_row(state, words_out); });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_constraint_counts(const KjarniHipConstraint* constraint, uint32_t* counts_out)
{
    if (!constraint || !counts_out) return KJARNI_ERROR_NULL_POINTER;
    const std::vector<uint32_t>& c = constraint->inner->counts();
    std::memcpy(counts_out, c.data(), c.size() * sizeof(uint32_t));
    return KJARNI_OK;
}

// ---- the kernels alone -----------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_constraint_mask(int32_t device, const uint16_t* trans, int32_t states, const uint32_t* tok_off,
                                                            const uint8_t* tok_bytes, int32_t vocab, uint64_t* mask_out, uint32_t* counts_out)
{
    if (!trans || !tok_off || !mask_out || !counts_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        if (states < 1 || states > kConstraintMaxStates) throw InvalidConfig("states must be 1.." + std::to_string(kConstraintMaxStates));
        check_table(tok_off, vocab);
        const size_t n_bytes = tok_off[vocab];
        if (n_bytes && !tok_bytes) throw InvalidConfig("tok_bytes is NULL but tok_off names " + std::to_string(n_bytes) + " bytes");
        for (size_t i = 0; i < (size_t)states * 256; ++i)
            if (trans[i] != kConstraintDead && trans[i] >= states) throw InvalidConfig("trans names a state that does not exist");
        const size_t words = ((size_t)vocab + 63) / 64, mask_bytes = (size_t)states * words * 8;
        if (mask_bytes > kConstraintMaxMaskBytes) throw InvalidConfig("the mask would need " + std::to_string(mask_bytes) + " bytes (limit 256 MiB)");
        use_device(device);
        DevBuf dt((size_t)states * 512), doff(((size_t)vocab + 1) * 4), dbytes(n_bytes);
        Guarded dmask(mask_bytes), dcount((size_t)states * 4);
        hip_check(hipMemcpy(dt.p, trans, (size_t)states * 512, hipMemcpyHostToDevice), "H2D table");
        hip_check(hipMemcpy(doff.p, tok_off, ((size_t)vocab + 1) * 4, hipMemcpyHostToDevice), "H2D offsets");
        if (n_bytes) hip_check(hipMemcpy(dbytes.p, tok_bytes, n_bytes, hipMemcpyHostToDevice), "H2D bytes");
        hip_check(hipMemset(dmask.buf.p, 0xAB, mask_bytes), "memset mask");  // (every word must be stored: nothing of this may survive)
        hip_check(hipMemset(dcount.buf.p, 0, (size_t)states * 4), "memset counts");
        hip_check(launch_constraint_mask(dt.as<uint16_t>(), states, doff.as<uint32_t>(), dbytes.as<uint8_t>(), vocab,
                                         dmask.as<unsigned long long>(), dcount.as<uint32_t>(), nullptr), "constraint mask");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(mask_out, dmask.buf.p, mask_bytes, hipMemcpyDeviceToHost), "D2H mask");
        hip_check(hipMemcpy(counts_out, dcount.buf.p, (size_t)states * 4, hipMemcpyDeviceToHost), "D2H counts");
        dmask.check("constraint mask");
        dcount.check("constraint counts");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_constraint_apply(int32_t device, const KjarniHipConstraint* constraint, const float* logits, int32_t rows,
                                                             int64_t ld, const uint32_t* states, const int32_t* done, const uint32_t* stop_ids,
                                                             int32_t n_stop, float* logits_out)
{
    if (!constraint || !logits || !states || !done || !logits_out || (n_stop > 0 && !stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const DeviceConstraint& c = *constraint->inner;
        const int vocab = c.vocab();
        if (rows < 1 || rows > 64 || ld < vocab) throw InvalidConfig("invalid apply dimensions (rows 1..64, ld >= vocab)");
        if (device != c.device()) throw InvalidConfig("the constraint lives on another device");
        for (int32_t r = 0; r < rows; ++r)
            if (states[r] >= (uint32_t)c.dfa().states()) throw InvalidConfig("states[" + std::to_string(r) + "] is no state of the automaton");
        const ConstraintView view = c.view(stop_list(stop_ids, n_stop));
        use_device(device);
        std::vector<ConstraintRow> rs((size_t)rows);
        for (int32_t r = 0; r < rows; ++r) rs[(size_t)r] = ConstraintRow{states[r], done[r] ? 1 : 0, 0, 0};
        const size_t bytes = (size_t)rows * (size_t)ld * 4;
        Guarded lg(bytes);
        DevBuf dv(sizeof(view)), dr(rs.size() * sizeof(ConstraintRow));
        hip_check(hipMemcpy(lg.buf.p, logits, bytes, hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemcpy(dv.p, &view, sizeof(view), hipMemcpyHostToDevice), "H2D view");
        hip_check(hipMemcpy(dr.p, rs.data(), rs.size() * sizeof(ConstraintRow), hipMemcpyHostToDevice), "H2D row state");
        hip_check(launch_constraint_apply(lg.as<float>(), ld, rows, vocab, dv.as<ConstraintView>(), dr.as<ConstraintRow>(), nullptr), "constraint apply");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(logits_out, lg.buf.p, bytes, hipMemcpyDeviceToHost), "D2H logits");
        lg.check("constrained logits");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_constraint_advance(int32_t device, const KjarniHipConstraint* constraint, const int32_t* picked,
                                                               int32_t rows, uint32_t* states, int32_t* done, const uint32_t* stop_ids,
                                                               int32_t n_stop, int32_t* violated_out)
{
    if (!constraint || !picked || !states || !done || !violated_out || (n_stop > 0 && !stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const DeviceConstraint& c = *constraint->inner;
        if (rows < 1 || rows > 4096) throw InvalidConfig("rows must be 1..4096");
        if (device != c.device()) throw InvalidConfig("the constraint lives on another device");
        for (int32_t r = 0; r < rows; ++r)
            if (states[r] >= (uint32_t)c.dfa().states()) throw InvalidConfig("states[" + std::to_string(r) + "] is no state of the automaton");
        const ConstraintView view = c.view(stop_list(stop_ids, n_stop));
        use_device(device);
        std::vector<ConstraintRow> rs((size_t)rows);
        for (int32_t r = 0; r < rows; ++r) rs[(size_t)r] = ConstraintRow{states[r], done[r] ? 1 : 0, 0, 0};
        Guarded dr(rs.size() * sizeof(ConstraintRow));
        DevBuf dv(sizeof(view)), dp((size_t)rows * 4);
        hip_check(hipMemcpy(dr.buf.p, rs.data(), rs.size() * sizeof(ConstraintRow), hipMemcpyHostToDevice), "H2D row state");
        hip_check(hipMemcpy(dv.p, &view, sizeof(view), hipMemcpyHostToDevice), "H2D view");
        hip_check(hipMemcpy(dp.p, picked, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D picks");
        hip_check(launch_constraint_advance(dp.as<int32_t>(), rows, dv.as<ConstraintView>(), dr.as<ConstraintRow>(), nullptr, nullptr, 0, nullptr),
                  "constraint advance");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(rs.data(), dr.buf.p, rs.size() * sizeof(ConstraintRow), hipMemcpyDeviceToHost), "D2H row state");
        dr.check("constraint row state");
        for (int32_t r = 0; r < rows; ++r) {
            states[r] = rs[(size_t)r].state;
            done[r] = rs[(size_t)r].done;
            violated_out[r] = rs[(size_t)r].violated;
        }
    });
}
