// C ABI of the lanes' constrained-decoding kernels alone (kjarni_hip.h): one launcher call of lane_constraint_kernels.h on host
// arrays.  Error conventions as ffi_grammar.cpp: NULL arguments are NULL_POINTER, everything else goes through guarded(), every
// refusal is made before a device is asked for, and every device buffer a kernel writes has a guard band behind it.
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kjarni_hip.h"
#include "ffi_common.h"
#include "ffi_constraint.h"
#include "ffi_grammar.h"
#include "host_util.h"
#include "lane_constraint_kernels.h"

using namespace kjarni;

static_assert(sizeof(KjarniHipLaneState) == sizeof(LlmLaneState) && KJARNI_HIP_BATCH_LANES == kMaxLanes, "the header's lane state is the kernels'");
static_assert(sizeof(KjarniHipWideState) == sizeof(LlmWideState) && KJARNI_HIP_WIDE_LANES == kLaneAutomatonSlots, "the header's wide state is the kernels'");

namespace {

// A device buffer with a guard band behind it (ffi_grammar.cpp's Guarded): check() throws when a kernel wrote past the end.
struct Guarded {
    static constexpr uint32_t kGuard = 0x7fc0beefu;
    static constexpr size_t kGuardWords = 64;
    size_t bytes;
    void* p = nullptr;
    explicit Guarded(size_t b) : bytes((b + 7) / 8 * 8)
    {
        hip_check(hipMalloc(&p, bytes + kGuardWords * 4), "hipMalloc");
        hip_check(hipMemsetD32((hipDeviceptr_t)((char*)p + bytes), (int)kGuard, kGuardWords), "guard band");
    }
    ~Guarded()
    {
        if (p) (void)hipFree(p);
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    void put(const void* host, size_t n, const char* what) const { hip_check(hipMemcpy(p, host, n, hipMemcpyHostToDevice), what); }
    void get(void* host, size_t n, const char* what) const { hip_check(hipMemcpy(host, p, n, hipMemcpyDeviceToHost), what); }
    void check(const char* what) const
    {
        uint32_t g[kGuardWords];
        hip_check(hipMemcpy(g, (char*)p + bytes, sizeof(g), hipMemcpyDeviceToHost), "D2H guard band");
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

// The table of an op call: the slots of lanes [first, first + lanes) from the caller's arrays, every other slot kind 0.  Every
// row must be a state / configuration of its lane's automaton, over `vocab` tokens, on `device`.
void make_table(LaneAutomatonTable& t, int32_t device, int32_t vocab, int32_t lanes, int32_t first, const int32_t* kinds,
                const KjarniHipConstraint* const* constraints, const KjarniHipGrammarConstraint* const* grammars, const uint32_t* states,
                const int32_t* depths, const uint16_t* stacks, const int32_t* done, const uint32_t* stop_ids, const int32_t* n_stop)
{
    std::memset(&t, 0, sizeof(t));
    for (int32_t l = first; l < first + lanes; ++l) {
        const std::string who = "lane " + std::to_string(l) + ": ";
        LaneAutomatonSlot& s = t.slot[l];
        if (kinds[l] < 0 || kinds[l] > 2) throw InvalidConfig(who + "kinds must be 0 (none), 1 (pattern) or 2 (grammar)");
        if (n_stop[l] < 0 || n_stop[l] > kConstraintMaxStops) throw InvalidConfig(who + "n_stop must be 0.." + std::to_string(kConstraintMaxStops));
        const std::vector<uint32_t> stops(stop_ids + (size_t)l * kConstraintMaxStops, stop_ids + (size_t)l * kConstraintMaxStops + n_stop[l]);
        s.kind = kinds[l];
        if (kinds[l] == kLaneKindPattern) {
            if (!constraints || !constraints[l]) throw InvalidConfig(who + "kind 1 needs constraints[lane]");
            const DeviceConstraint& c = *constraints[l]->inner;
            if (c.device() != device) throw InvalidConfig(who + "the constraint lives on another device");
            if (c.vocab() != vocab) throw InvalidConfig(who + "the constraint's token table has " + std::to_string(c.vocab()) + " tokens, the call's vocab is " + std::to_string(vocab));
            if (states[l] >= (uint32_t)c.dfa().states()) throw InvalidConfig(who + "states is no state of the automaton");
            s.cview = c.view(stops);
            s.crow.state = states[l];
            s.crow.done = done[l] ? 1 : 0;
        } else if (kinds[l] == kLaneKindGrammar) {
            if (!grammars || !grammars[l]) throw InvalidConfig(who + "kind 2 needs grammars[lane]");
            const DeviceGrammar& g = *grammars[l]->inner;
            if (g.device() != device) throw InvalidConfig(who + "the grammar constraint lives on another device");
            if (g.vocab() != vocab) throw InvalidConfig(who + "the grammar's token table has " + std::to_string(g.vocab()) + " tokens, the call's vocab is " + std::to_string(vocab));
            if (states[l] >= (uint32_t)g.grammar().states()) throw InvalidConfig(who + "states is no state of the automaton");
            if (depths[l] < 0 || depths[l] > kGrammarMaxDepth) throw InvalidConfig(who + "depths must be 0.." + std::to_string(kGrammarMaxDepth));
            s.gview = g.view(stops);
            s.grow.state = states[l];
            s.grow.depth = depths[l];
            s.grow.done = done[l] ? 1 : 0;
            std::memcpy(s.grow.stack, stacks + (size_t)l * kGrammarMaxDepth, sizeof(s.grow.stack));  // (all 64 words: those above depth must survive)
            for (int32_t i = 0; i < depths[l]; ++i)
                if (s.grow.stack[i] >= g.grammar().states()) throw InvalidConfig(who + "stacks[" + std::to_string(i) + "] is no state of the automaton");
        }
    }
}

void check_range(int32_t lanes, int32_t first, int32_t limit, int64_t ld, int32_t vocab)
{
    if (lanes < 1 || first < 0 || first > limit - lanes)
        throw InvalidConfig("lanes [first_lane, first_lane + lanes) must lie in 0.." + std::to_string(limit) + " with at least one lane");
    if (vocab < 1 || ld < vocab || ld > (1 << 20)) throw InvalidConfig("vocab >= 1, vocab <= ld <= 2^20");
}

}  // namespace

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_lane_automaton_apply(int32_t device, const float* logits, int64_t ld, int32_t vocab, int32_t lanes,
                                                                 int32_t first_lane, const int32_t* live, const int32_t* kinds,
                                                                 const KjarniHipConstraint* const* constraints,
                                                                 const KjarniHipGrammarConstraint* const* grammars, const uint32_t* states,
                                                                 const int32_t* depths, const uint16_t* stacks, const int32_t* done,
                                                                 const uint32_t* stop_ids, const int32_t* n_stop, float* logits_out)
{
    if (!logits || !live || !kinds || !states || !depths || !stacks || !done || !stop_ids || !n_stop || !logits_out) return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        check_range(lanes, first_lane, kLaneAutomatonSlots, ld, vocab);
        std::vector<LaneAutomatonTable> table(1);
        make_table(table[0], device, vocab, lanes, first_lane, kinds, constraints, grammars, states, depths, stacks, done, stop_ids, n_stop);
        int32_t lv[kLaneAutomatonSlots] = {};
        for (int32_t l = first_lane; l < first_lane + lanes; ++l) lv[l] = live[l] ? 1 : 0;
        use_device(device);
        const size_t bytes = (size_t)(first_lane + lanes) * (size_t)ld * 4;
        Guarded lg(bytes), dt(sizeof(LaneAutomatonTable)), dl(sizeof(lv));
        lg.put(logits, bytes, "H2D logits");
        dt.put(table.data(), sizeof(LaneAutomatonTable), "H2D table");
        dl.put(lv, sizeof(lv), "H2D live");
        hip_check(launch_lane_automaton_apply(lg.as<float>(), ld, vocab, lanes, first_lane, dt.as<LaneAutomatonTable>(), dl.as<int32_t>(), nullptr),
                  "lane automaton apply");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        lg.check("lane-constrained logits");
        dt.check("lane automaton table");
        dl.check("live flags");
        std::vector<LaneAutomatonTable> after(1);
        dt.get(after.data(), sizeof(LaneAutomatonTable), "D2H table");
        if (std::memcmp(after.data(), table.data(), sizeof(LaneAutomatonTable)) != 0) throw std::runtime_error("the lane apply changed the automaton table");
        lg.get(logits_out, bytes, "D2H logits");
    });
}

KJARNI_EXPORT KjarniErrorCode kjarni_hip_op_lane_automaton_pick(int32_t device, int32_t wide, const float* logits, int64_t ld, int32_t vocab,
                                                                int32_t lanes, int32_t first_lane, void* state, int32_t* history,
                                                                int32_t hist_stride, int32_t capacity, int32_t advance, const int32_t* kinds,
                                                                const KjarniHipConstraint* const* constraints,
                                                                const KjarniHipGrammarConstraint* const* grammars, uint32_t* states,
                                                                int32_t* depths, uint16_t* stacks, int32_t* done, const uint32_t* stop_ids,
                                                                const int32_t* n_stop, int32_t* violated_out)
{
    if (!logits || !state || !history || !kinds || !states || !depths || !stacks || !done || !stop_ids || !n_stop || !violated_out)
        return KJARNI_ERROR_NULL_POINTER;
    return guarded(KJARNI_ERROR_INFERENCE_FAILED, [&] {
        const int set_lanes = wide ? kMaxWideLanes : kMaxLanes;
        check_range(lanes, first_lane, set_lanes, ld, vocab);
        if (hist_stride < 1 || hist_stride > (1 << 16) || capacity < 0) throw InvalidConfig("hist_stride 1..2^16, capacity >= 0");
        // the fields of either layout, lane by lane
        int32_t* base = static_cast<int32_t*>(state);
        int32_t *s_live = base + 2 * set_lanes, *s_count = base + 3 * set_lanes, *s_nstop = base + 5 * set_lanes;
        for (int l = first_lane; l < first_lane + lanes; ++l) {
            if (s_nstop[l] < 0 || s_nstop[l] > kMaxLaneStops) throw InvalidConfig("n_stop[" + std::to_string(l) + "] of the state must be 0..16");
            if (s_live[l] && (s_count[l] < 0 || s_count[l] >= hist_stride))
                throw InvalidConfig("count[" + std::to_string(l) + "] is no entry of the lane's history");
        }
        std::vector<LaneAutomatonTable> table(1);
        make_table(table[0], device, vocab, lanes, first_lane, kinds, constraints, grammars, states, depths, stacks, done, stop_ids, n_stop);
        for (int l = 0; l < set_lanes; ++l) table[0].slot[l].walked = s_count[l];  // every pick so far has been walked
        use_device(device);
        const size_t sb = wide ? sizeof(LlmWideState) : sizeof(LlmLaneState);
        const size_t lb = (size_t)(first_lane + lanes) * (size_t)ld * 4, hb = (size_t)set_lanes * (size_t)hist_stride * 4;
        Guarded dl(lb), sd(sb), hd(hb), best(kMaxWideLanes * sizeof(unsigned long long)), dt(sizeof(LaneAutomatonTable));
        dl.put(logits, lb, "H2D logits");
        sd.put(state, sb, "H2D state");
        hd.put(history, hb, "H2D history");
        dt.put(table.data(), sizeof(LaneAutomatonTable), "H2D table");
        hip_check(hipMemset(best.p, 0, kMaxWideLanes * sizeof(unsigned long long)), "memset");
        hip_check(launch_lane_automaton_pick(dl.as<float>(), ld, vocab, lanes, first_lane, best.as<unsigned long long>(),
                                             LaneStateRef::at(sd.p, set_lanes), hd.as<int32_t>(), hist_stride, capacity, advance ? 1 : 0,
                                             dt.as<LaneAutomatonTable>(), nullptr), wide ? "wide automaton pick" : "lane automaton pick");
        hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        dl.check("logits"); sd.check("lane state"); hd.check("lane history"); best.check("pick scratch"); dt.check("lane automaton table");
        unsigned long long b[kMaxWideLanes];
        best.get(b, sizeof(b), "D2H best");
        for (int i = 0; i < kMaxWideLanes; ++i)
            if (b[i] != 0ull) throw std::runtime_error("the pick left its accumulator non-zero");
        std::vector<LaneAutomatonTable> after(1);
        dt.get(after.data(), sizeof(LaneAutomatonTable), "D2H table");
        sd.get(state, sb, "D2H state");
        hd.get(history, hb, "D2H history");
        for (int32_t l = first_lane; l < first_lane + lanes; ++l) {
            const LaneAutomatonSlot& s = after[0].slot[l];
            violated_out[l] = 0;
            if (s.kind == kLaneKindPattern) {
                states[l] = s.crow.state;
                done[l] = s.crow.done;
                violated_out[l] = s.crow.violated;
            } else if (s.kind == kLaneKindGrammar) {
                states[l] = s.grow.state;
                depths[l] = s.grow.depth;
                done[l] = s.grow.done;
                violated_out[l] = s.grow.violated;
                std::memcpy(stacks + (size_t)l * kGrammarMaxDepth, s.grow.stack, sizeof(s.grow.stack));
            }
        }
    });
}
