// C ABI of grammar-constrained decoding (kjarni_hip.h): the grammar compiler and the host walk (no GPU), the device object, and
// the two kernels alone on logits and row states given by the host.  Error conventions as ffi_constraint.cpp: NULL arguments are
// NULL_POINTER, everything else goes through guarded(), and every refusal is made before any GPU work.
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kjarni_hip.h"
#include "ffi_common.h"
#include "ffi_grammar.h"
#include "host_util.h"

using namespace kjarni;

static_assert(KJARNI_GRAMMAR_MAX_RULES == kGrammarMaxRules, "header constant");
static_assert(KJARNI_GRAMMAR_MAX_STATES == kGrammarMaxStates, "header constant");
static_assert(KJARNI_GRAMMAR_MAX_DEPTH == kGrammarMaxDepth, "header constant");
static_assert(KJARNI_GRAMMAR_TOKEN_PUSHES == kGrammarTokenPushes, "header constant");
static_assert(sizeof(GrammarRow) == 16 + 2 * kGrammarMaxDepth, "GrammarRow layout");

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

// An output buffer with a guard band behind it (ffi_constraint.cpp's Guarded): check() throws when a kernel wrote past the end.
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

std::vector<uint32_t> stop_list(const uint32_t* stop_ids, int32_t n_stop)
{
    if (n_stop < 0 || n_stop > kConstraintMaxStops)
        throw InvalidConfig("n_stop must be 0.." + std::to_string(kConstraintMaxStops) + ", got " + std::to_string(n_stop));
    return std::vector<uint32_t>(stop_ids, stop_ids + n_stop);
}

// The rows of an op call as the device holds them; every row must be a configuration of the automaton.
std::vector<GrammarRow> make_rows(const Grammar& g, int32_t rows, const uint32_t* states, const int32_t* depths, const uint16_t* stacks, const int32_t* done)
{
    std::vector<GrammarRow> rs((size_t)rows);
    for (int32_t r = 0; r < rows; ++r) {
        GrammarRow& row = rs[(size_t)r];
        if (states[r] >= (uint32_t)g.states()) throw InvalidConfig("states[" + std::to_string(r) + "] is no state of the automaton");
        if (depths[r] < 0 || depths[r] > kGrammarMaxDepth)
            throw InvalidConfig("depths[" + std::to_string(r) + "] must be 0.." + std::to_string(kGrammarMaxDepth));
        row.state = states[r];
        row.depth = depths[r];
        row.done = done[r] ? 1 : 0;
        row.violated = 0;
        std::memcpy(row.stack, stacks + (size_t)r * kGrammarMaxDepth, sizeof(row.stack));  // (all 64 words: those above depth must survive)
        for (int32_t i = 0; i < depths[r]; ++i)
            if (row.stack[i] >= g.states()) throw InvalidConfig("stacks[" + std::to_string(r) + "][" + std::to_string(i) + "] is no state of the automaton");
    }
    return rs;
}

}  // namespace

// ---- the compiler and the walk (no GPU) ------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_compile(const char* const* names, const char* const* patterns, int32_t n_rules, KjarniHipGrammar** out)
{
    if (!names || !patterns || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    for (int32_t r = 0; r < n_rules && r <= kGrammarMaxRules; ++r)
        if (!names[r] || !patterns[r]) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INVALID_CONFIG, [&] {
        if (n_rules < 1) throw InvalidConfig("grammar: no rule (rule 0 is the start rule)");
        if (n_rules > kGrammarMaxRules) throw InvalidConfig("grammar: " + std::to_string(n_rules) + " rules, the limit is " + std::to_string(kGrammarMaxRules));
        std::vector<std::pair<std::string, std::string>> rules;
        for (int32_t r = 0; r < n_rules; ++r) rules.emplace_back(names[r], patterns[r]);
        auto h = std::make_unique<KjarniHipGrammar>();
        try {
            h->grammar = compile_grammar(rules);
        } catch (const GrammarError& e) {
            throw InvalidConfig(e.what());
        }
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_grammar_free(KjarniHipGrammar* grammar) { delete grammar; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_dims(const KjarniHipGrammar* grammar, int32_t* states, int32_t* rules)
{
    if (!grammar) return KJARNI_ERROR_NULL_POINTER;
    if (states) *states = grammar->grammar.states();
    if (rules) *rules = (int32_t)grammar->grammar.rules.size();
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_table(const KjarniHipGrammar* grammar, uint32_t* action_out, uint8_t* flags_out, uint16_t* rule_of_out)
{
    if (!grammar) return KJARNI_ERROR_NULL_POINTER;
    const Grammar& g = grammar->grammar;
    if (action_out) std::memcpy(action_out, g.action.data(), g.action.size() * sizeof(uint32_t));
    if (flags_out) std::memcpy(flags_out, g.flags.data(), g.flags.size());
    if (rule_of_out) std::memcpy(rule_of_out, g.rule_of.data(), g.rule_of.size() * sizeof(uint16_t));
    return KJARNI_OK;
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_walk(const KjarniHipGrammar* grammar, uint32_t state, const uint16_t* stack, int32_t depth,
                                                      const uint8_t* bytes, size_t n, int32_t as_token, uint32_t* state_out, uint16_t* stack_out,
                                                      int32_t* depth_out, int32_t* alive_out)
{
    if (!grammar || !state_out || !stack_out || !depth_out || !alive_out || (n && !bytes) || (depth > 0 && !stack)) return KJARNI_ERROR_NULL_POINTER;
    GrammarConfig c;
    c.state = state;
    c.depth = depth;
    if (depth > 0 && depth <= kGrammarMaxDepth) std::memcpy(c.stack, stack, (size_t)depth * sizeof(uint16_t));
    *alive_out = grammar->grammar.walk(&c, bytes, n, as_token != 0) ? 1 : 0;
    if (*alive_out) {
        *state_out = c.state;
        *depth_out = c.depth;
        std::memcpy(stack_out, c.stack, (size_t)c.depth * sizeof(uint16_t));
    }
    return KJARNI_OK;
}

// ---- the device object -----------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_constraint_new(int32_t device, const KjarniHipGrammar* grammar, const uint32_t* tok_off,
                                                                const uint8_t* tok_bytes, int32_t vocab, KjarniHipGrammarConstraint** out)
{
    if (!grammar || !tok_off || !out) return KJARNI_ERROR_NULL_POINTER;
    *out = nullptr;
    return guarded(KJARNI_ERROR_LOAD_FAILED, [&] {
        if (vocab < 1) throw InvalidConfig("vocab must be at least 1");
        if (tok_off[0] != 0) throw InvalidConfig("tok_off[0] must be 0");
        for (int32_t t = 0; t < vocab; ++t)
            if (tok_off[t + 1] < tok_off[t]) throw InvalidConfig("tok_off decreases at token " + std::to_string(t));
        if (tok_off[vocab] && !tok_bytes) throw InvalidConfig("tok_bytes is NULL but tok_off names " + std::to_string(tok_off[vocab]) + " bytes");
        TokenTable table;
        table.off.assign(tok_off, tok_off + vocab + 1);
        if (tok_off[vocab]) table.bytes.assign(tok_bytes, tok_bytes + tok_off[vocab]);
        auto h = std::make_unique<KjarniHipGrammarConstraint>();
        h->inner = std::make_unique<DeviceGrammar>(device, grammar->grammar, std::move(table));
        *out = h.release();
    });
}

KJARNI_EXPORT void kjarni_hip_grammar_constraint_free(KjarniHipGrammarConstraint* constraint) { delete constraint; }

KJARNI_EXPORT KjarniErrorCode kjarni_hip_grammar_constraint_dims(const KjarniHipGrammarConstraint* constraint, int32_t* states, int32_t* vocab)
{
    if (!constraint) return KJARNI_ERROR_NULL_POINTER;
    if (states) *states = constraint->inner->grammar().states();
    if (vocab) *vocab = constraint->inner->vocab();
    return KJARNI_OK;
}

// ---- the kernels alone -----------------------------------------------------------------------------------------------------------

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_grammar_apply(int32_t device, const KjarniHipGrammarConstraint* constraint, const float* logits, int32_t rows,
                                                          int64_t ld, const uint32_t* states, const int32_t* depths, const uint16_t* stacks,
                                                          const int32_t* done, const uint32_t* stop_ids, int32_t n_stop, float* logits_out)
{
    if (!constraint || !logits || !states || !depths || !stacks || !done || !logits_out || (n_stop > 0 && !stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const DeviceGrammar& c = *constraint->inner;
        const int vocab = c.vocab();
        if (rows < 1 || rows > 64 || ld < vocab) throw InvalidConfig("invalid apply dimensions (rows 1..64, ld >= vocab)");
        if (device != c.device()) throw InvalidConfig("the grammar constraint lives on another device");
        const std::vector<GrammarRow> rs = make_rows(c.grammar(), rows, states, depths, stacks, done);
        const GrammarView view = c.view(stop_list(stop_ids, n_stop));
        use_device(device);
        const size_t bytes = (size_t)rows * (size_t)ld * 4;
        Guarded lg(bytes);
        DevBuf dv(sizeof(view)), dr(rs.size() * sizeof(GrammarRow));
        hip_check(hipMemcpy(lg.buf.p, logits, bytes, hipMemcpyHostToDevice), "H2D logits");
        hip_check(hipMemcpy(dv.p, &view, sizeof(view), hipMemcpyHostToDevice), "H2D view");
        hip_check(hipMemcpy(dr.p, rs.data(), rs.size() * sizeof(GrammarRow), hipMemcpyHostToDevice), "H2D row state");
        hip_check(launch_grammar_apply(lg.as<float>(), ld, rows, vocab, dv.as<GrammarView>(), dr.as<GrammarRow>(), nullptr), "grammar apply");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(logits_out, lg.buf.p, bytes, hipMemcpyDeviceToHost), "D2H logits");
        lg.check("grammar-constrained logits");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_grammar_advance(int32_t device, const KjarniHipGrammarConstraint* constraint, const int32_t* picked, int32_t rows,
                                                            uint32_t* states, int32_t* depths, uint16_t* stacks, int32_t* done, const uint32_t* stop_ids,
                                                            int32_t n_stop, int32_t* violated_out, int32_t log_count, int32_t log_cap,
                                                            uint32_t* state_log, int32_t* depth_log)
{
    if (!constraint || !picked || !states || !depths || !stacks || !done || !violated_out || (n_stop > 0 && !stop_ids)) return KJARNI_ERROR_NULL_POINTER;
    if (log_cap > 0 && (!state_log || !depth_log)) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const DeviceGrammar& c = *constraint->inner;
        if (rows < 1 || rows > 4096) throw InvalidConfig("rows must be 1..4096");
        if (log_cap < 0 || log_cap > 4096 || (log_cap > 0 && rows != 1)) throw InvalidConfig("the log takes one row and at most 4096 entries");
        if (device != c.device()) throw InvalidConfig("the grammar constraint lives on another device");
        std::vector<GrammarRow> rs = make_rows(c.grammar(), rows, states, depths, stacks, done);
        const GrammarView view = c.view(stop_list(stop_ids, n_stop));
        use_device(device);
        const size_t cap = (size_t)log_cap;
        Guarded dr(rs.size() * sizeof(GrammarRow)), dsl(cap * 4), ddl(cap * 4);
        DevBuf dv(sizeof(view)), dp((size_t)rows * 4), dc(4);
        hip_check(hipMemcpy(dr.buf.p, rs.data(), rs.size() * sizeof(GrammarRow), hipMemcpyHostToDevice), "H2D row state");
        hip_check(hipMemcpy(dv.p, &view, sizeof(view), hipMemcpyHostToDevice), "H2D view");
        hip_check(hipMemcpy(dp.p, picked, (size_t)rows * 4, hipMemcpyHostToDevice), "H2D picks");
        hip_check(hipMemcpy(dc.p, &log_count, 4, hipMemcpyHostToDevice), "H2D count");
        if (cap) {
            hip_check(hipMemcpy(dsl.buf.p, state_log, cap * 4, hipMemcpyHostToDevice), "H2D state log");
            hip_check(hipMemcpy(ddl.buf.p, depth_log, cap * 4, hipMemcpyHostToDevice), "H2D depth log");
        }
        hip_check(launch_grammar_advance(dp.as<int32_t>(), rows, dv.as<GrammarView>(), dr.as<GrammarRow>(), cap ? dsl.as<uint32_t>() : nullptr,
                                         cap ? ddl.as<int32_t>() : nullptr, cap ? dc.as<int>() : nullptr, log_cap, nullptr), "grammar advance");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        hip_check(hipMemcpy(rs.data(), dr.buf.p, rs.size() * sizeof(GrammarRow), hipMemcpyDeviceToHost), "D2H row state");
        if (cap) {
            hip_check(hipMemcpy(state_log, dsl.buf.p, cap * 4, hipMemcpyDeviceToHost), "D2H state log");
            hip_check(hipMemcpy(depth_log, ddl.buf.p, cap * 4, hipMemcpyDeviceToHost), "D2H depth log");
        }
        dr.check("grammar row state");
        dsl.check("grammar state log");
        ddl.check("grammar depth log");
        for (int32_t r = 0; r < rows; ++r) {
            const GrammarRow& row = rs[(size_t)r];
            states[r] = row.state;
            depths[r] = row.depth;
            done[r] = row.done;
            violated_out[r] = row.violated;
            std::memcpy(stacks + (size_t)r * kGrammarMaxDepth, row.stack, sizeof(row.stack));
        }
    });
}
