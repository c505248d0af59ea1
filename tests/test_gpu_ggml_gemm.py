"""The GGUF prompt GEMM (launch_prefill_gemm_ggml through kjarni_hip_op_prefill_gemm_ggml) against float64 over the dequantized
weights at the project's prompt-GEMM bar (fp8_gemm_ref64.bar: 1e-5 x max(1, max |ref|)), and whole GGUF models with
set_ggml_matrix_cores: forward(), the wide step and generate_wide against the float64 reference and against the switch off.
Every kernel call runs twice for the same bits, with NaN in every element it must not read (pad columns, a row past m) or write."""
import itertools
import os
import shutil

import numpy as np
import pytest

from tests import fp8_gemm_ref64 as R
from tests import gguf_fixture as G
from tests import prefill_ref64 as P
from tests import wide_cases as WC
from tests import wide_fp8_cases as FC
from tests.quant_proj_ref64 import ggml_weights64

pytestmark = pytest.mark.gpu
TYPES = {8: "Q8_0", 12: "Q4_K", 14: "Q6_K"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {}   # type -> the largest error seen, as a fraction of the bar (printed by the last kernel test)


def run(t, a, blocks, k, m, n, ldy=None, exact=None, **kw):
    """One call, twice: y (NaN wherever the kernel must not write), the gate, the slice count; checked against float64."""
    from kjarni_amd import ops
    ap = np.full((m + 1, k + 4), np.nan, np.float32)
    ap[:m, :k] = a
    y0 = np.full((m, n if ldy is None else ldy), np.nan, np.float32)
    if kw.get("r_is_y"):
        y0[:, :n] = kw.pop("r0")
    outs = [ops.prefill_gemm_ggml(ap, blocks, t, k, m, y0, **kw) for _ in range(2)]
    y, gate, used = outs[0]
    assert np.array_equal(y, outs[1][0], equal_nan=True) and used == outs[1][2], "two runs differ"
    assert used == P.ksplit_rule(m, n, k, scratch=kw.get("split", True))
    assert np.isnan(y[:, n:]).all(), "columns past n were written"
    r = y0[:, :n] if kw.get("r_is_y") else kw.get("r")
    ref = P.gemm64(a, ggml_weights64(t, blocks, n, k), kw.get("bias"), None if r is None else r[:, :n], kw.get("gate"))
    got = y[:, :n]
    if kw.get("gate") is not None:
        assert np.array_equal(gate, outs[1][1])
        ref, got = ref[1], gate
    if exact:
        assert np.array_equal(got, ref.astype(np.float32)), "a one-hot probe is not the f32 product"
    err = float(np.abs(got - ref).max()) / R.bar(ref)
    WORST[t] = max(WORST.get(t, 0.0), err)
    assert err <= 1.0, (TYPES[t], m, n, k, err)
    return used


@pytest.mark.parametrize("k", [256, 512, 768, 2048])    # 768: four slices of 192 columns, boundaries inside the 256-blocks
@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_grid(t, k):
    rng = np.random.default_rng(100 * t + k)
    for n in (8, 64, 200):
        blocks = G.random_blocks(t, n, k, rng)
        for m in (1, 9, 64, 65, 130):
            run(t, rng.standard_normal((m, k)).astype(np.float32), blocks, k, m, n)
    assert P.ksplit_rule(64, 64, 768) == 4 and (768 // 4) % 256


def far_apart(t, n, k):
    """Blocks whose neighbouring sub-block scales lie far apart: d 2^6 apart from one 32-block (Q8_0) or 256-block (K-quants) to the
    next, and inside a 256-block the integer scales 1 | 32 (Q4_K: six bits hold no 2^6) or 1 | 64 (Q6_K) in turn; Q4_K with a nonzero
    min on alternate sub-blocks only."""
    rng = np.random.default_rng(t)
    b = G.random_blocks(t, n, k, rng).reshape(-1, G.BLOCK[t][1])
    d = np.where(np.arange(b.shape[0]) % 2, 2.0 ** -6, 2.0 ** -12).astype(np.float16).view(np.uint8).reshape(-1, 2)
    if t == 8:
        b[:, :2] = d
    elif t == 12:
        b[:, 0:2], b[:, 2:4] = d, d
        sc, mn = np.tile([1, 32], 4), np.tile([0, 37], 4)                # get_scale_min_k4 inverted
        q = [sc[j] | (sc[j + 4] >> 4) << 6 for j in range(4)] + [mn[j] | (mn[j + 4] >> 4) << 6 for j in range(4)]
        b[:, 4:16] = np.array(q + [(sc[j + 4] & 15) | (mn[j + 4] & 15) << 4 for j in range(4)], np.uint8)
    else:
        b[:, 208:210] = d
        b[:, 192:208] = np.tile(np.array([1, 64], np.int8), 8).view(np.uint8)
    return b.reshape(n, -1)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_scales_far_apart_and_one_hot_probes(t, split):
    rng = np.random.default_rng(t)
    for k, m in ((768, 65), (512, 9)):
        run(t, rng.standard_normal((m, k)).astype(np.float32), far_apart(t, 72, k), k, m, 72, split=split)
    # one 256-block pair, a one-hot row at the first and last k of every 16-element sub-block (so of every 32 and every slice)
    k, at = 512, np.sort(np.concatenate([np.arange(0, 512, 16), np.arange(15, 512, 16)]))
    a = np.zeros((64, k), np.float32)
    a[np.arange(64), at] = 1.0
    run(t, a, far_apart(t, 72, k), k, 64, 72, split=split, exact=t == 8)   # Q8_0: one f32 product d * q per output, bit for bit


@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_epilogues_and_layout(t):
    rng = np.random.default_rng(50 + t)
    m, n, k = 65, 200, 512
    a, blocks = rng.standard_normal((m, k)).astype(np.float32), G.random_blocks(t, n, k, rng)
    bias, r = rng.standard_normal(n).astype(np.float32), rng.standard_normal((m, n + 8)).astype(np.float32)
    gate = rng.standard_normal((m, n)).astype(np.float32)
    gate[::7, ::5], gate[1::7, ::5] = 90.0, -90.0                        # silu at +-90: no overflow, no NaN
    for split in (True, False):
        assert run(t, a, blocks, k, m, n, bias=bias, split=split) == (4 if split else 1)
        run(t, a, blocks, k, m, n, bias=bias, r=r, split=split)          # the residual apart, its own stride
        run(t, a, blocks, k, m, n, bias=bias, r_is_y=True, r0=r[:, :n], split=split)
        run(t, a, blocks, k, m, n, gate=gate, split=split)
        run(t, a, blocks, k, m, n, ldy=n + 96, bias=bias, split=split)   # a segment of wider rows: nothing past n written
    print("largest error / bar:", {TYPES[x]: round(v, 4) for x, v in WORST.items()})


# ---- whole models ----------------------------------------------------------------------------------------------------------------
QWEN = dict(G.QWEN_Q, max_position_embeddings=256)
MODELS = {   # name: (geometry, types, gguf_model arguments)
    "llama-q4km": (G.LLAMA_Q, G.q4_k_m_types(2), dict(seed=41, rope_freqs=True)),
    "llama-q8_0": (G.LLAMA_Q, {x: 8 for x in ("embed", "q", "k", "v", "o", "gate", "up", "down")}, dict(seed=42, rope_freqs=True)),
    "qwen2-q6k": (QWEN, {"embed": 8, "q": 12, "k": 8, "v": 14, "o": 12, "gate": 8, "up": 12, "down": 14}, dict(seed=43)),
}
# name: the prompts of wide_cases.prompts(0, vocab) whose float64 greedy runs are clear at every step (qwen3_ref64.assert_margins),
# found on the CPU with the reference alone; clear_greedy() asserts the margin again
CLEAR = {"llama-q4km": (0, 1, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 23, 24, 26, 27, 30, 31),
         "llama-q8_0": (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 22, 23, 24, 25, 26, 27),
         "qwen2-q6k": (0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 23, 24, 25, 26)}


TAU = 2e-4   # code units: 127 x sqrt(512) x 2^-24, the f32 rounding of a 512-term row against float64, on the Q8_K code scale


def reference(hf, cfg, types):
    """The float64 reference; the rows of a Q6_K linear go through Q8_K first (test_gpu_gguf._Ref64Q8K).  Q8_K rounds, so f32 rows
    that differ from the float64 rows in the last bits can land on the neighbouring code where |x / d| lies within TAU of k + 1/2:
    those elements are recorded in `near` as (distance, (call, row, column)), and the ones listed in `flip` round the other way."""
    from tests.llm_ref64 import Ref64
    from tests.test_gpu_gguf import _Ref64Q8K

    class FlipRef(_Ref64Q8K):
        calls, near, flip = 0, (), frozenset()

        def linear(self, x, name, layer):
            if (name, layer) not in self.q6k:
                return Ref64.linear(self, x, name, layer)
            q, d = G.q8k_quantize(x.astype(np.float32))
            d3 = np.repeat(d, 256, axis=1)
            a = np.abs(np.divide(x.astype(np.float32), d3, out=np.zeros(x.shape, np.float32), where=d3 != 0)).astype(np.float64)
            for r, c in zip(*np.nonzero(np.abs(a % 1 - 0.5) < TAU)):
                self.near.append((abs(a[r, c] % 1 - 0.5), (self.calls, r, c)))
                if (self.calls, r, c) in self.flip:
                    q[r, c] = np.sign(x[r, c]) * (2 * np.floor(a[r, c]) + 1 - abs(q[r, c]))
            self.calls += 1
            return Ref64.linear(self, q * d3.astype(np.float64), name, layer)

    names = {"q": "q_proj", "k": "k_proj", "v": "v_proj", "o": "o_proj", "gate": "gate_proj", "up": "up_proj", "down": "down_proj"}
    q6k = {(names[key.split(".")[0]], layer) for key, t in types.items() if t == 14 and key.split(".")[0] in names
           for layer in ([int(key.split(".")[1])] if "." in key else range(cfg["num_hidden_layers"]))}
    return FlipRef(hf, cfg, q6k)


def lane64(ref, blocks, flip=()):
    """The logits after each block of ids of one sequence, from an empty cache, with the codes in `flip` rounded the other way."""
    ref.calls, ref.near, ref.flip, cache = 0, [], frozenset(flip), ref.new_cache()
    return [FC.logits64(ref, ref.forward(b, cache)[-1:])[0] for b in blocks]


def close_or_flipped(ref, blocks, got, what):
    """got[i] against the float64 logits after blocks[i] at the decoder's bar -- or against the reference with one of its eight (or two of its
    four) nearest-to-a-boundary Q8_K codes rounded the other way (a model with Q6_K linears; reference())."""
    def ok(want):
        return all(g is None or np.abs(g - w).max() <= 1e-4 * max(1.0, np.abs(w).max()) for g, w in zip(got, want))
    if ok(lane64(ref, blocks)):
        return
    near = [key for _, key in sorted(ref.near)[:8]]
    assert any(ok(lane64(ref, blocks, f)) for f in [(k,) for k in near] + list(itertools.combinations(near[:4], 2))), what


@pytest.fixture(scope="module", params=MODELS)
def model(request, tmp_path_factory):
    import kjarni_amd
    geometry, types, kw = MODELS[request.param]
    path = str(tmp_path_factory.mktemp(request.param) / "model.gguf")
    cfg, hf = G.gguf_model(path, geometry, types, **kw)
    ps, news = WC.prompts(0, cfg["vocab_size"]), WC.max_new(0)
    return kjarni_amd.HipDecoder(path), reference(hf, cfg, types), cfg, path, [(ps[i], news[i]) for i in CLEAR[request.param]]


def close(got, want, what, rows_off=0):
    bad = (np.abs(got - want).reshape(len(got), -1).max(axis=1) > 1e-4 * max(1.0, np.abs(want).max())).sum()
    assert bad <= rows_off, (what, int(bad))


def test_forward_switch_on_against_float64_and_switch_off(model):
    dec, ref, cfg, _, _ = model
    dec.set_ggml_matrix_cores(False)
    ids = np.random.default_rng(3).integers(4, cfg["vocab_size"], 130).tolist()
    for n in (24, 64, 130):
        outs = []
        for on in (False, True):
            dec.set_ggml_matrix_cores(on)
            assert dec.ggml_matrix_cores() is on
            dec.reset()
            outs.append(dec.forward(ids[:n]))
        close_or_flipped(ref, [ids[:n]], [outs[1][1]], ("float64", n))
        close(outs[1][1][None], outs[0][1][None], ("switch off", n))
        # the last eight hidden rows: with Q6_K linears one row may hold a Q8_K code that the two routes round apart
        close(outs[1][0], outs[0][0], ("hidden rows", n), rows_off=1 if ref.q6k else 0)


@pytest.mark.parametrize("lanes", [9, 64])
def test_wide_step_and_generate_wide(model, lanes):
    dec, ref, cfg, _, clear = model
    dec.set_ggml_matrix_cores(False)
    with pytest.raises(Exception, match="more than 8 lanes do not take a quantized \\(GGUF\\) checkpoint: the prompt GEMM would dequantize"):
        dec.generate_wide([p for p, _ in clear[:9]], 4, lanes=9, lane_context=WC.LANE_CONTEXT)   # off: the refusal as it was
    dec.set_ggml_matrix_cores(True)
    rng = np.random.default_rng(lanes)
    prompts = [rng.integers(4, cfg["vocab_size"], int(rng.integers(2, 30))).tolist() for _ in range(lanes)]
    dec.wide_begin(lanes, WC.LANE_CONTEXT)
    for lane, p in enumerate(prompts):
        dec.wide_prefill(lane, p[:-1])
    steps = [[p[-1] for p in prompts], rng.integers(4, cfg["vocab_size"], lanes).tolist()]
    logits = [dec.wide_step(toks)[1] for toks in steps]                  # the wide step itself: every lane's logits against float64
    for lane, p in enumerate(prompts):
        close_or_flipped(ref, [p[:-1], [steps[0][lane]], [steps[1][lane]]], [None, logits[0][lane], logits[1][lane]], ("wide step", lane))
    reqs = [clear[i % len(clear)] for i in range(lanes + 8)]             # more requests than lanes: the lanes turn over
    want = {id(p): FC.clear_greedy(ref, cfg, p, m, "reference") for p, m in clear}   # asserts the margin at every step
    got = dec.generate_wide([p for p, _ in reqs], [m for _, m in reqs], lanes=lanes, lane_context=WC.LANE_CONTEXT)
    dec.set_ggml_matrix_cores(False)
    for (p, m), g in zip(reqs, got):
        assert g == want[id(p)] == dec.generate(p, m), p


def test_f32_load_ignores_the_switch_and_fp8_switch_is_a_no_op(model):
    import kjarni_amd
    dec, _, cfg, path, _ = model
    dec.set_ggml_matrix_cores(False)
    dec.set_fp8_matrix_cores(True)
    assert not dec.fp8_matrix_cores() and not dec.ggml_matrix_cores()
    f = kjarni_amd.HipDecoder(path, weights="f32")
    ids = list(range(4, 70))
    before = f.forward(ids)[1]
    f.set_ggml_matrix_cores(True)
    f.reset()
    assert not f.ggml_matrix_cores() and np.array_equal(f.forward(ids)[1], before)


def test_generator_and_chat_carry_the_switch(tmp_path):
    from kjarni_amd import Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    d = tmp_path / "gguf"
    G.gguf_model(str(d / "model.gguf"), dict(G.LLAMA_Q, vocab_size=720, bos_token_id=700, eos_token_id=701), G.q4_k_m_types(2), seed=13, rope_freqs=True)
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), str(d / "tokenizer.json"))
    cfg = GenerationConfig(do_sample=False, max_new_tokens=8)
    message = "Is water wet? Answer in one short sentence, and say why you think so."      # more than 24 tokens: the prompt route
    texts = [f"{message} {i}" for i in range(12)]
    for obj, call in ((Chat("llama3.2-1b-instruct", model_path=str(d)), lambda o: o.send(message, cfg)),
                      (Generator("llama3.2-1b-instruct", model_path=str(d)), lambda o: o.generate_batch(texts, cfg))):
        plain = call(obj)
        obj.set_ggml_matrix_cores(True)
        if isinstance(obj, Generator):
            obj.set_wide_lanes(16)                                       # 12 texts on the wide bank: refused with the switch off
        assert call(obj) == plain
        obj.set_ggml_matrix_cores(False)
