"""Wide lanes: 9..64 prompts decoded in lock step with every projection on the prompt GEMM's 64-row tile
(kjarni_hip_decoder_generate_wide, its hooks, kjarni_hip_op_wide_rope_scatter / _wide_pick, Generator.set_wide_lanes).

The two per-lane kernels alone against float64 and the pick rule; wide steps against the float64 references, ragged, with
frozen lanes and a lane that fills its cache; a row's independence of the width; generate_wide against generate() and the
references on the 72-prompt sets of tests/wide_cases.py; stop ids, callbacks, processors, prefix reuse, a qwen3_moe model,
the refusals.  Float bar: the decoder's, max |gpu - ref| <= 1e-4 * max(1, max |ref|); the scatter alone: 1e-5 (one rotation in
f32, a 128-term sum of squares at most); ids are compared only where the reference's two best logits are lanes_cases.GAP apart."""

import numpy as np
import pytest

from oracle import llm_oracle as L
from tests import dense_proj_ref64 as D
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import llm_ref64, synth
from tests import token_select_cases as TS
from tests import wide_cases as WC
from tests.gpt2_ref64 import Gpt2Ref64
from tests.qwen3_ref64 import Qwen3Ref64

pytestmark = pytest.mark.gpu
TOL = 1e-4
STEPS = 5
NAN = np.float32(np.nan)


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _within(got, ref, what):
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), _bar(ref)
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- the scatter alone ------------------------------------------------------------------------------------------------------------

def _rope_tables(rows, d, seed):
    ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, (rows, d // 2))
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _head_norm64(v, heads, d, gamma, eps):
    h = np.asarray(v, np.float64).reshape(heads, d)
    return (h / np.sqrt(np.mean(h * h, axis=1, keepdims=True) + eps) * np.asarray(gamma, np.float64)).reshape(-1)


@pytest.mark.parametrize("form", ["rotate", "copy", "qwen3"])
@pytest.mark.parametrize("d,heads,kvh", [(16, 4, 1), (64, 8, 2), (128, 4, 4)], ids=["d16-mqa", "d64-gqa", "d128-mha"])
@pytest.mark.parametrize("lanes", [9, 33, 64])
def test_scatter_alone_against_float64(lanes, d, heads, kvh, form):
    from kjarni_amd import ops
    rng = np.random.default_rng(1000 * lanes + d)
    cap, lane_rows = 12, 14                                  # two rows of every lane lie past the capacity
    qd, kv = heads * d, kvh * d
    width, ld = qd + 2 * kv, qd + 2 * kv + 4               # four pad columns behind Q | K | V
    cos_t, sin_t = _rope_tables(cap, d, lanes)
    pos = rng.integers(1, cap - 1, lanes).astype(np.int32)
    live = np.ones(lanes, np.int32)
    pos[0], pos[1], pos[2] = 0, cap - 1, cap                 # first row, last row, a lane stopped at its capacity
    live[[3, lanes - 2]] = 0                                 # frozen lanes, one of them in the last pair
    pos[lanes - 1] = cap - 1
    qkv = np.full((lanes, ld), NAN, np.float32)
    qkv[:, :width] = rng.standard_normal((lanes, width)).astype(np.float32) * 2
    qkv[live == 0] = NAN                                     # nothing of a frozen lane may be read into anything compared
    kc, vc = np.full((lanes, lane_rows, kv), NAN, np.float32), np.full((lanes, lane_rows, kv), NAN, np.float32)
    gq = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32) if form == "qwen3" else None
    gk = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32) if form == "qwen3" else None
    eps = 1e-6
    kw = dict(rotate=form != "copy", gamma_q=gq, gamma_k=gk, eps=eps)
    q1, k1, v1 = ops.wide_rope_scatter(qkv, heads, kvh, d, cos_t, sin_t, kc, vc, cap, pos, live, **kw)
    q2, k2, v2 = ops.wide_rope_scatter(qkv, heads, kvh, d, cos_t, sin_t, kc, vc, cap, pos, live, **kw)
    assert _same_bits(q1, q2) and _same_bits(k1, k2) and _same_bits(v1, v2), "the same call twice differs"
    for l in range(lanes):
        p, on = int(pos[l]), bool(live[l]) and pos[l] < cap
        assert _same_bits(q1[l, qd:], qkv[l, qd:]), f"lane {l}: K | V | pad of the staging row changed"
        touched = np.zeros(lane_rows, bool)
        if not on:
            assert _same_bits(q1[l], qkv[l]), f"lane {l}: a lane that writes nothing had its Q changed"
        else:
            touched[p] = True
            q_in, k_in, v_in = qkv[l, :qd], qkv[l, qd:qd + kv], qkv[l, qd + kv:width]
            if form == "qwen3":
                q_ref = D.rope64(_head_norm64(q_in, heads, d, gq, eps), heads, d, cos_t[p], sin_t[p])
                k_ref = D.rope64(_head_norm64(k_in, kvh, d, gk, eps), kvh, d, cos_t[p], sin_t[p])
            elif form == "rotate":
                q_ref, k_ref = D.rope64(q_in, heads, d, cos_t[p], sin_t[p]), D.rope64(k_in, kvh, d, cos_t[p], sin_t[p])
            else:
                q_ref, k_ref = q_in.astype(np.float64), k_in.astype(np.float64)
            for name, got, ref in (("q", q1[l, :qd], q_ref), ("k", k1[l, p], k_ref)):
                err = float(np.abs(got.astype(np.float64) - ref).max())
                assert err <= D.bar(ref), f"lane {l} {name}: {err:.3e} > {D.bar(ref):.3e}"
            assert _same_bits(v1[l, p], v_in), f"lane {l}: V is not the copy"
            if form == "copy":
                assert _same_bits(k1[l, p], k_in) and _same_bits(q1[l, :qd], q_in)
        for name, got in (("k", k1), ("v", v1)):             # every other cache row still holds its NaN pattern
            assert _same_bits(got[l][~touched], kc[l][~touched]), f"lane {l}: {name} rows outside pos were written"


# ---- the pick alone ---------------------------------------------------------------------------------------------------------------

def _state(lanes):
    from kjarni_amd import _ffi
    return _ffi.KjarniHipWideState()


@pytest.mark.parametrize("vocab", [320, 151936])
@pytest.mark.parametrize("lanes", [9, 64])
def test_pick_alone_against_the_rule(lanes, vocab):
    from kjarni_amd import ops
    cases = TS.argmax_cases(vocab)
    rows = np.stack([cases[l % len(cases)][1] for l in range(lanes)])       # ties, the two zeros, -inf rows ... cycled over the lanes
    want = [TS.last_max(rows[l]) for l in range(lanes)]
    stride, cap, UNT = 6, 40, -77
    frozen, limited, stop_lanes, full = 4, 5, (0, lanes - 1), 6
    st = _state(lanes)
    hist = np.full((64, stride), UNT, np.int32)
    for l in range(64):
        st.token[l], st.pos[l], st.count[l], st.limit[l] = UNT - l, 10 + (l % 7), l % 3, 1 << 20
        st.live[l] = int(l < lanes and l != frozen)
    st.limit[limited] = st.count[limited] + 1                                # this pick is the lane's last
    st.pos[full] = cap - 1                                                   # the advance fills the lane's cache
    for l in stop_lanes:                                                     # the pick is one of the lane's stop ids (the last of three)
        st.n_stop[l] = 3
        st.stop[l][0], st.stop[l][1], st.stop[l][2] = vocab + 5, (want[l] + 1) % vocab, want[l]
    st.n_stop[7] = 16                                                        # sixteen stop ids, none of them the pick
    for e in range(16):
        st.stop[7][e] = (want[7] + 1 + e) % vocab
    before = {f: [getattr(st, f)[l] for l in range(64)] for f in ("token", "pos", "live", "count", "limit", "n_stop")}
    out = ops.wide_pick(rows, st, hist, cap, advance=True)
    for l in range(64):
        cnt, live0 = before["count"][l], before["live"][l]
        if not live0:
            assert [getattr(st, f)[l] for f in before] == [before[f][l] for f in before], f"lane {l}: a frozen lane's state changed"
            assert (out[l] == UNT).all(), f"lane {l}: a frozen lane's history changed"
            continue
        assert out[l, cnt] == want[l], f"lane {l} ({cases[l % len(cases)][0]}): picked {out[l, cnt]}, the rule gives {want[l]}"
        assert (np.delete(out[l], cnt) == UNT).all(), f"lane {l}: wrote outside its history entry"
        assert st.count[l] == cnt + 1 and st.pos[l] == before["pos"][l] + 1
        ends = l in stop_lanes or l == limited or l == full
        assert st.live[l] == int(not ends), f"lane {l}: live = {st.live[l]}"
        assert st.token[l] == (before["token"][l] if ends else want[l])
    # the prefill pick: one lane, no advance
    st2 = _state(lanes)
    st2.live[lanes - 1], st2.limit[lanes - 1], st2.pos[lanes - 1] = 1, 5, 3
    out2 = ops.wide_pick(rows, st2, np.full((64, stride), UNT, np.int32), cap, lanes=1, first_lane=lanes - 1, advance=False)
    assert out2[lanes - 1, 0] == want[lanes - 1] and (out2[:lanes - 1] == UNT).all()
    assert st2.pos[lanes - 1] == 3 and st2.count[lanes - 1] == 1 and st2.token[lanes - 1] == want[lanes - 1] and st2.live[lanes - 1] == 1


# ---- wide steps against float64 ---------------------------------------------------------------------------------------------------

class _LlamaRef:
    def __init__(self, t, cfg):
        self.orc, self.r64, self.vocab, self.first_id = L.LlmOracle(t, cfg), llm_ref64.Ref64(t, cfg), cfg["vocab_size"], 4

    def new(self):
        return [self.orc.new_cache(), self.r64.new_cache()]

    def forward(self, ids, state):
        self.r64.forward(ids, state[1])
        h = self.orc.forward(ids, state[0])[0][-1]
        return h, self.orc.logits(h)

    def cache(self, state):
        return state[1]


class _Gpt2Ref:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = Gpt2Ref64(t, cfg), cfg["vocab_size"], 0

    def new(self):
        return self.ref.new_cache()

    def forward(self, ids, state):
        h, lg = self.ref.forward(list(ids), state)
        return h[-1], lg

    def cache(self, state):
        return state


class _Qwen3Ref:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = Qwen3Ref64(t, cfg), cfg["vocab_size"], 4

    def new(self):
        return self.ref.new_cache()

    def forward(self, ids, state):
        h = self.ref.forward(ids, state)[-1:]
        return self.ref.final_norm(h)[0], self.ref.logits(h)[0]

    def cache(self, state):
        return state


def _model(tmp_path, family, seed=3, bf16=False):
    """(decoder, reference, context) of a tiny model of the family; bf16: the matrices stored (and referenced) as bf16 values."""
    from kjarni_amd import HipDecoder
    d = str(tmp_path / f"{family}-{seed}-{int(bf16)}")
    if family == "gpt2":
        cfg = G.gpt2_config(**G.SMALL)
        _, t = G.gpt2_model(d, cfg, seed=seed, store_bf16=bf16)
        return HipDecoder(d, 0), _Gpt2Ref(t, cfg), cfg["n_ctx"]
    if family == "qwen3":
        from tests import qwen3_fixture as Q3
        cfg, t = Q3.qwen3_model(d, Q3.Q3_SMALL, seed=seed, store_bf16=bf16)
        return HipDecoder(d, 0), _Qwen3Ref(t, cfg), cfg["max_position_embeddings"]
    base = synth.LLAMA_TEST if family == "llama" else synth.QWEN_TEST
    cfg, t = synth.llm_model(d, base, seed=seed, store_bf16=bf16)
    return HipDecoder(d, 0), _LlamaRef(t, cfg), cfg["max_position_embeddings"]


def _check_caches(dec, ref, states, lanes, what):
    for l in lanes:
        cache = ref.cache(states[l])
        assert dec.wide_cache_len(l) == cache[0][0].shape[0], f"{what}: lane {l} length"
        got = [dec.wide_kv_rows(l, i) for i in range(len(cache))]
        for (layer, name), (err, bar) in llm_ref64.cache_errors(got, cache).items():
            assert err <= bar, f"{what}: lane {l} layer {layer} {name}: {err:.3e} > {bar:.3e}"


LENS = [1, 2, 7, 8, 23, 24, 40]


def _run_wide_steps(dec, ref, n, seed, lane_context=64, freeze=()):
    """test_gpu_llm_lanes._run_lane_steps on the wide hooks: n lanes with prompt lengths cycled from LENS, lane 5 two tokens
    short of its capacity; every live lane's hidden row, logits row and K / V rows are compared at every step."""
    rng = np.random.default_rng(seed)
    dec.wide_begin(n, lane_context)
    cap = dec.wide_capacity()
    assert cap == lane_context
    lens = [LENS[l % len(LENS)] for l in range(n)]
    lens[5] = cap - 2
    states = [ref.new() for _ in range(n)]
    for l, m in enumerate(lens):
        ids = rng.integers(ref.first_id, ref.vocab, m).tolist()
        ref.forward(ids, states[l])
        dec.wide_prefill(l, ids)
    _check_caches(dec, ref, states, range(n), "after prefill")
    frozen_rows = {}
    for step in range(STEPS):
        live = [int(dec.wide_cache_len(l) < cap and not (l in freeze and step >= 3)) for l in range(n)]
        for l in range(n):
            if not live[l] and l not in frozen_rows:
                frozen_rows[l] = (dec.wide_cache_len(l), [dec.wide_kv_rows(l, i) for i in range(dec.layers)])
        ids = rng.integers(ref.first_id, ref.vocab, n).tolist()
        hidden, logits = dec.wide_step(ids, live)
        for l in range(n):
            if live[l]:
                h_ref, l_ref = ref.forward([ids[l]], states[l])
                _within(hidden[l], h_ref, f"step {step} lane {l} hidden")
                _within(logits[l], l_ref, f"step {step} lane {l} logits")
        _check_caches(dec, ref, states, [l for l in range(n) if live[l]], f"step {step}")
    for l, (length, rows) in frozen_rows.items():
        assert dec.wide_cache_len(l) == length, f"frozen lane {l} grew"
        for i in range(dec.layers):
            k, v = dec.wide_kv_rows(l, i)
            assert _same_bits(k, rows[i][0]) and _same_bits(v, rows[i][1]), f"frozen lane {l} layer {i} rewritten"
    _check_caches(dec, ref, states, range(n), "after the steps")
    return frozen_rows


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", ["llama", "qwen2", "gpt2", "qwen3"])
def test_wide_steps_against_float64_ragged(tmp_path, family, bf16):
    dec, ref, ctx = _model(tmp_path, family, bf16=bf16)
    assert dec.bf16 == bf16 and ctx >= 64
    for n in (9, 16, 33, 64):
        freeze = (2, 7, n - 1)
        frozen = _run_wide_steps(dec, ref, n, seed=n, freeze=freeze)
        assert set(freeze) | {5} <= set(frozen) and frozen[5][0] == 64      # lane 5 stopped at its capacity, the others were frozen


@pytest.mark.parametrize("family", ["llama", "gpt2"])
def test_a_row_does_not_depend_on_its_neighbours(tmp_path, family):
    """The same nine lanes at widths 9 and 64 (the other 55 lanes hold other prompts): one M-tile and one K split either
    way, so the same bits are expected; asserted is the float bar, the bit equality is reported."""
    dec, ref, _ = _model(tmp_path, family)
    rng = np.random.default_rng(5)
    prompts = [rng.integers(ref.first_id, ref.vocab, LENS[l % len(LENS)]).tolist() for l in range(64)]
    steps = [rng.integers(ref.first_id, ref.vocab, 64).tolist() for _ in range(3)]
    got = {}
    for n in (9, 64):
        dec.wide_begin(n, 64)
        for l in range(n):
            dec.wide_prefill(l, prompts[l])
        got[n] = [dec.wide_step(ids[:n])[1][:9].copy() for ids in steps]
    equal = all(_same_bits(a, b) for a, b in zip(got[9], got[64]))
    print(f"{family}: logits rows at widths 9 and 64 bit-equal: {equal}")
    for s, (a, b) in enumerate(zip(got[9], got[64])):
        _within(a, b.astype(np.float64), f"step {s}: width 9 against width 64")


# ---- generate_wide ----------------------------------------------------------------------------------------------------------------

def _case(tmp_path, case):
    from kjarni_amd import HipDecoder
    seed, cfg, t, ps, news = WC.case_set(case)
    d = str(tmp_path / case)
    WC.write_model(case, seed, d)
    exp, gap = WC.reference_runs(case, cfg, t, ps, news)
    assert gap >= LC.GAP, f"precondition: the reference's two best logits come within {gap:.2e}"
    assert len(ps) == WC.N_PROMPTS and all(4 <= m <= 10 for m in news)
    return HipDecoder(d, 0), cfg, ps, news, exp


@pytest.mark.parametrize("case", ["llama", "qwen2", "qwen3", "gpt2"])
def test_generate_wide_equals_single_stream_and_the_reference(tmp_path, case):
    dec, cfg, ps, news, exp = _case(tmp_path, case)
    single = [dec.generate(p, m) for p, m in zip(ps, news)]
    assert single == exp
    for lanes in (9, 64, 0):                                               # 72 prompts: every width turns lanes over
        assert dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT) == exp, lanes
    # eight lanes or fewer are generate_batch's route: the same ids, by the same step
    s0 = dec.lane_gemv_calls()
    assert dec.generate_wide(ps, news, lanes=8, lane_context=WC.LANE_CONTEXT) == dec.generate_batch(ps, news, lanes=8, lane_context=WC.LANE_CONTEXT) == exp
    assert dec.generate_wide(ps[:5], news[:5], lanes=64, lane_context=WC.LANE_CONTEXT) == dec.generate_batch(ps[:5], news[:5], lane_context=WC.LANE_CONTEXT)
    assert sum(dec.lane_gemv_calls()) > sum(s0)                            # (the GEMV step ran)
    s1 = dec.lane_gemv_calls()
    assert dec.generate_wide(ps[:20], news[:20], lanes=16, lane_context=WC.LANE_CONTEXT) == exp[:20]
    assert dec.lane_gemv_calls() == s1                                     # (the wide step takes no GEMV)
    assert [dec.generate(p, m) for p, m in zip(ps, news)] == single        # a plain generate() afterwards


def test_stop_ids_end_wide_lanes_at_different_steps(tmp_path):
    dec, cfg, ps, news, exp = _case(tmp_path, "eos")
    ends = WC.stopped(exp, ps, news)
    assert len(ends) >= WC.EOS_MIN_STOPPED and len(set(ends.values())) >= 2, ends
    for lanes in (16, 64):
        got = dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT)
        assert got == exp, lanes
        assert all(tok not in cfg["eos_token_id"] for ids in got for tok in ids)
    assert exp == [dec.generate(p, m) for p, m in zip(ps, news)]


def test_wide_callbacks_step_major_and_cancel_one_prompt(tmp_path):
    dec, cfg, ps, news, exp = _case(tmp_path, "llama")
    ps, news, exp = ps[:12], news[:12], exp[:12]
    seen = []
    got = dec.generate_wide(ps, news, lanes=12, lane_context=WC.LANE_CONTEXT, on_token=lambda i, t: seen.append((i, t)))
    assert got == exp
    order = [(s, i) for s in range(max(news)) for i in range(12) if s < len(exp[i])]
    assert seen == [(i, exp[i][s]) for s, i in order]                      # step order, lane order within a step
    cut = 2
    count = [0] * 12

    def cancel_third(i, t):                                                # False on prompt 3's third token ends that prompt only
        count[i] += 1
        return not (i == 3 and count[i] == cut + 1)
    got = dec.generate_wide(ps, news, lanes=12, lane_context=WC.LANE_CONTEXT, on_token=cancel_third)
    assert len(exp[3]) > cut + 1
    assert got[3] == exp[3][:cut + 1] and got[:3] + got[4:] == exp[:3] + exp[4:]


def test_processors_in_wide_lanes_equal_prompt_by_prompt(tmp_path):
    dec, cfg, ps, news, exp = _case(tmp_path, "processors")
    single = [dec.generate(p, m, **WC.PROCESSORS) for p, m in zip(ps, news)]
    assert single == exp
    for lanes in (9, 64):
        assert dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT, **WC.PROCESSORS) == exp, lanes


def test_prefix_reuse_in_wide_lanes(tmp_path):
    dec, cfg, ps, news, exp = _case(tmp_path, "llama")
    prefix = np.random.default_rng(77).integers(4, cfg["vocab_size"], 24).tolist()
    ps, news = [prefix + p[:12] for p in ps[:20]], news[:20]
    off = dec.generate_wide(ps, news, lanes=16, lane_context=WC.LANE_CONTEXT)
    assert off == [dec.generate(p, m) for p, m in zip(ps, news)]
    dec.set_prefix_reuse(True)
    dec.reset()
    r0, c0 = dec.prefix_stats()
    assert dec.generate_wide(ps, news, lanes=16, lane_context=WC.LANE_CONTEXT) == off
    r1, c1 = dec.prefix_stats()
    shared = 24                                                             # (the prompts differ right behind the prefix)
    assert all(len(p) > 24 for p in ps) and len({p[24] for p in ps}) > 1
    assert c1 - c0 == shared + sum(len(p) - shared for p in ps), "the prefix is computed once"
    assert r1 - r0 == shared * len(ps)
    # the prefix rows of a lane are the single-sequence cache's, bit for bit
    dec.wide_begin(16, WC.LANE_CONTEXT)
    dec.reset()
    dec.forward(prefix)
    dec.wide_prefill_shared(9, 24, ps[0][24:])
    assert dec.wide_cache_len(9) == len(ps[0])
    for i in range(dec.layers):
        k, v = dec.wide_kv_rows(9, i, 0, 24)
        k0, v0 = dec.kv_rows(i, 0, 24)
        assert _same_bits(k, k0) and _same_bits(v, v0), f"layer {i}: the copied prefix rows differ"
    dec.set_prefix_reuse(False)


def test_qwen3_moe_in_wide_lanes(tmp_path):
    """The MoE rows hook inside the wide step (captured: launch_moe_ffn_grouped reads nothing back).  Twenty prompts whose
    float64 runs are clear at every routed token and every greedy step, asserted here again."""
    from kjarni_amd import HipDecoder
    from tests import moe_fixture as M
    d = str(tmp_path / "moe")
    cfg, t = M.moe_model(d, M.MOE_SMALL)
    dec = HipDecoder(d, 0)
    ps = WC.moe_prompts(cfg["vocab_size"])
    assert len(ps) == 20
    want = [WC.moe_clear_greedy(t, cfg, p, f"prompt {i}") for i, p in enumerate(ps)]
    assert [dec.generate(p, WC.MOE_NEW) for p in ps] == want
    assert dec.generate_wide(ps, WC.MOE_NEW, lanes=16, lane_context=WC.LANE_CONTEXT) == want
    sparse = [i for i in range(cfg["num_hidden_layers"]) if i not in cfg.get("mlp_only_layers", [])]
    ids, w = dec.moe_routing(sparse[-1])
    assert ids.shape == (16, cfg["num_experts_per_tok"]) and w.shape == ids.shape   # the last wide step's record: a row per lane
    assert ((ids >= 0) & (ids < cfg["num_experts"])).all() and np.isfinite(w).all()


# ---- refusals on the device -----------------------------------------------------------------------------------------------------------

def test_quantized_and_fp8_checkpoints_are_refused_above_eight_lanes(tmp_path):
    from kjarni_amd import HipDecoder
    from kjarni_amd._ffi import KjarniError, KjarniException
    from tests import fp8_fixture as F
    from tests import gguf_fixture as GG
    path = str(tmp_path / "q" / "model.gguf")
    qcfg, _ = GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    fcfg, _ = F.fp8_model(str(tmp_path / "f"), dict(synth.LLAMA_TEST), "tensor", seed=2)
    for d, vocab, word in ((str(tmp_path / "q"), qcfg["vocab_size"], "quantized"), (str(tmp_path / "f"), fcfg["vocab_size"], "FP8")):
        dec = HipDecoder(d)
        ps = LC.prompts(3, vocab, n=9)
        with pytest.raises(KjarniException) as e:
            dec.generate_wide(ps, 3, lanes=9, lane_context=64)
        assert e.value.code == KjarniError.INVALID_CONFIG and word in str(e.value) and "dequantize" in str(e.value)
        with pytest.raises(KjarniException) as e:
            dec.wide_begin(9, 64)
        assert e.value.code == KjarniError.INVALID_CONFIG
        assert dec.generate_wide(ps, 3, lanes=8, lane_context=64) == [dec.generate(p, 3) for p in ps]


def test_wide_begin_refuses_eight_lanes_and_the_hooks_check_their_ranges(tmp_path):
    from kjarni_amd._ffi import KjarniError, KjarniException
    dec, ref, _ = _model(tmp_path, "llama")
    for lanes in (8, 1, 65, -1):
        with pytest.raises(KjarniException) as e:
            dec.wide_begin(lanes, 64)
        assert e.value.code == KjarniError.INVALID_CONFIG
    dec.wide_begin(9, 32)
    assert dec.wide_capacity() == 32 and dec.wide_cache_len(9) == -1 and dec.wide_cache_len(8) == 0
    with pytest.raises(KjarniException):
        dec.wide_prefill(9, [5, 6])
    with pytest.raises(KjarniException):
        dec.wide_prefill(0, list(range(4, 37)))                             # 33 tokens into 32 rows
    with pytest.raises(KjarniException) as e:
        dec.generate_batch([[5]] * 9, 2, lanes=9)
    assert e.value.code == KjarniError.INVALID_CONFIG                       # the lanes route keeps its 1..8


def test_generate_wide_refusals_name_the_argument_and_write_nothing(tmp_path):
    from kjarni_amd import HipDecoder
    import ctypes as C

    from kjarni_amd import _ffi
    from kjarni_amd._ffi import KjarniError, KjarniException, lib
    dec, ref, _ = _model(tmp_path, "llama")
    ps = LC.prompts(1, ref.vocab, n=12)
    for kw, word in ((dict(lanes=65), "lanes"), (dict(lanes=-1), "lanes")):
        with pytest.raises(KjarniException) as e:
            dec.generate_wide(ps, 4, lane_context=64, **kw)
        assert e.value.code == KjarniError.INVALID_CONFIG and word in e.value.message
    for width in (12, 4):                                                   # the wide route and the forwarded one refuse alike
        bad = [list(p) for p in ps[:width]]
        bad[2] = []
        with pytest.raises(KjarniException) as e:
            dec.generate_wide(bad, 4, lanes=width, lane_context=64)
        assert e.value.code == KjarniError.INVALID_CONFIG and "empty prompt (prompt 2)" in e.value.message
        bad[2] = list(range(4, 4 + 65))                                     # 65 tokens into 64 rows
        with pytest.raises(KjarniException) as e:
            dec.generate_wide(bad, 4, lanes=width, lane_context=64)
        assert e.value.code == KjarniError.INVALID_CONFIG and "prompt 2" in e.value.message
    # the outputs of a refused call are untouched (n_out is zeroed before the checks, as generate_batch does)
    flat = np.arange(4, 16, dtype=np.uint32)
    off = (C.c_size_t * 13)(*range(13))
    new = (C.c_size_t * 12)(*[3] * 12)
    out = np.full((12, 3), 99, np.uint32)
    n_out = (C.c_size_t * 12)(*[7] * 12)
    code = lib().kjarni_hip_decoder_generate_wide(dec._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), off, 12, new, 1.0, 0, 65, 64,
                                                  _ffi.KjarniBatchTokenCallbackFn(), None,
                                                  out.ctypes.data_as(C.POINTER(C.c_uint32)), 3, n_out)
    assert code == KjarniError.INVALID_CONFIG and (out == 99).all() and list(n_out) == [0] * 12
    # seventeen stop ids
    d = str(tmp_path / "stops")
    synth.llm_model(d, dict(synth.LLAMA_TEST, eos_token_id=list(range(40, 57))), seed=1)
    many = HipDecoder(d, 0)
    with pytest.raises(KjarniException) as e:
        many.generate_wide(ps, 4, lanes=12, lane_context=64)
    assert e.value.code == KjarniError.INVALID_CONFIG and "16 stop ids" in e.value.message


# ---- Generator ----------------------------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


def _generator(tmp_path):
    from kjarni_amd import Generator
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    return Generator("gpt2", model_path=d)


def test_generator_set_wide_lanes(tmp_path):
    from kjarni_amd._ffi import KjarniException
    from kjarni_amd.chat import GenerationConfig
    gen = _generator(tmp_path)
    texts = TEXTS * 3
    greedy = GenerationConfig(do_sample=False, max_new_tokens=12)
    single = [gen.generate(text, greedy) for text in TEXTS] * 3
    assert gen.generate_batch(texts, greedy) == single
    gen.set_wide_lanes(16)
    assert gen.generate_batch(texts, greedy) == single                     # fifteen texts: fifteen wide lanes
    gen.set_wide_lanes(0)
    assert gen.generate_batch(texts, greedy) == single                     # off: the lanes path again
    with pytest.raises(KjarniException):
        gen.set_lanes(9)
    with pytest.raises(KjarniException):
        gen.set_wide_lanes(65)


def test_sampling_in_wide_lanes(tmp_path):
    """top_k = 1 is greedy; a seeded run repeats; and it gives the same texts at widths 16 and 64 (every request draws from
    its own generator, seeded in request order at call start) -- which also needs a row of the M <= 64 GEMM not to depend on
    the rows beside it."""
    from kjarni_amd.chat import GenerationConfig
    gen = _generator(tmp_path)
    texts = [f"{t} {i}" for i in range(14) for t in TEXTS]                # 70 texts: 64 lanes turn over
    gen.set_wide_lanes(64)
    greedy = gen.generate_batch(texts, GenerationConfig(do_sample=False, max_new_tokens=8))
    assert gen.generate_batch(texts, GenerationConfig(do_sample=True, top_k=1, max_new_tokens=8)) == greedy
    hot = GenerationConfig(do_sample=True, temperature=1.5, max_new_tokens=8)
    runs = []
    for lanes in (16, 16, 64):
        gen.set_wide_lanes(lanes)
        gen.seed(1234)
        runs.append(gen.generate_batch(texts, hot))
    assert runs[0] == runs[1], "a seeded run does not repeat"
    assert runs[0] == runs[2], "a seeded run differs between widths 16 and 64"
    assert runs[0] != greedy
