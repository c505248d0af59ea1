"""The affine-32 prompt GEMM (launch_prefill_gemm_affine through kjarni_hip_op_prefill_gemm_affine) against float64 over the
host-dequantized weights at the project's prompt-GEMM bar (fp8_gemm_ref64.bar: 1e-5 x max(1, max |ref|)), and the three models of
test_gpu_gguf_affine with set_affine_matrix_cores: forward() and generate_wide against the float64 reference and the switch off.
Every kernel call runs twice for the same bits, with NaN in every element it must not read (pad columns, a row past m) or write.

Largest kernel error seen on one MI355X, as a fraction of the bar: Q4_0 0.021, Q4_1 0.016, Q5_0 0.015, Q5_1 0.018, Q5_K 0.020."""
import os
import shutil

import numpy as np
import pytest

from tests import fp8_gemm_ref64 as R
from tests import gguf_fixture as G
from tests import gguf_types_fixture as T
from tests import prefill_ref64 as P
from tests import wide_cases as WC
from tests import wide_fp8_cases as FC
from tests.test_gpu_ggml_gemm import TAU, reference
from tests.test_gpu_gguf_affine import ALL, MODELS, check_greedy, close, logits_of

pytestmark = pytest.mark.gpu
TYPES = {t: name for name, t in T.NEW_TYPES.items()}
EXACT = (T.Q4_0, T.Q5_0)   # b' = 0: the fold of a one-hot row is the one exact product a * (q - c), the f32 weight itself
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {}   # type -> the largest error seen, as a fraction of the bar (printed by the last kernel test)


def run(t, a, blocks, k, m, n, ldy=None, exact=False, **kw):
    """One call, twice: y (NaN wherever the kernel must not write), the gate, the slice count; checked against float64."""
    from kjarni_amd import ops
    ap = np.full((m + 1, k + 4), np.nan, np.float32)
    ap[:m, :k] = a
    y0 = np.full((m, n if ldy is None else ldy), np.nan, np.float32)
    if kw.get("r_is_y"):
        y0[:, :n] = kw.pop("r0")
    outs = [ops.prefill_gemm_affine(ap, blocks, t, k, m, y0, **kw) for _ in range(2)]
    y, gate, used = outs[0]
    assert np.array_equal(y, outs[1][0], equal_nan=True) and used == outs[1][2], "two runs differ"
    assert used == P.ksplit_rule(m, n, k, scratch=kw.get("split", True))
    assert np.isnan(y[:, n:]).all(), "columns past n were written"
    r = y0[:, :n] if kw.get("r_is_y") else kw.get("r")
    ref = P.gemm64(a, T.dequantize(t, blocks, n, k), kw.get("bias"), None if r is None else r[:, :n], kw.get("gate"))
    got = y[:, :n]
    if kw.get("gate") is not None:
        assert np.array_equal(gate, outs[1][1])
        ref, got = ref[1], gate
    if exact:
        assert np.array_equal(got, ref.astype(np.float32)), "a one-hot probe is not the f32 weight"
    err = float(np.abs(got - ref).max()) / R.bar(ref)
    WORST[t] = max(WORST.get(t, 0.0), err)
    print(TYPES[t], (m, n, k), "error / bar", round(err, 4))
    assert err <= 1.0, (TYPES[t], m, n, k, err)
    return used


@pytest.mark.parametrize("t,k", [(t, k) for t in TYPES for k in (32, 224, 512, 768, 2048) if t != T.Q5_K or k % 256 == 0],
                         ids=lambda v: TYPES.get(v, str(v)))
def test_grid(t, k):   # 768: four slices of 192 columns; 224: unsplit
    rng = np.random.default_rng(100 * t + k)
    for n in (8, 64, 200):
        blocks = T.random_blocks(t, n, k, rng)
        for m in (1, 9, 64, 65, 130):
            run(t, rng.standard_normal((m, k)).astype(np.float32), blocks, k, m, n)
    assert P.ksplit_rule(64, 64, 768) == 4 and P.ksplit_rule(64, 64, 224) == 1


def far_apart(t, n, k):
    """Blocks whose neighbouring runs have scales 2^6 apart (Q5_K: d from one 256-block to the next, and the integer scales 1 | 32 in
    turn inside it: six bits hold no 2^6); Q4_1 / Q5_1 / Q5_K with a nonzero offset on alternate runs only."""
    b = T.random_blocks(t, n, k, np.random.default_rng(t)).reshape(-1, T.BLOCK[t][1])
    odd = np.arange(b.shape[0]) % 2
    b[:, 0:2] = np.where(odd, 2.0 ** -6, 2.0 ** -12).astype(np.float16).view(np.uint8).reshape(-1, 2)
    if t in (T.Q4_1, T.Q5_1):
        b[:, 2:4] = np.where(odd, -0.11, 0.0).astype(np.float16).view(np.uint8).reshape(-1, 2)
    elif t == T.Q5_K:
        b[:, 2:4] = b[:, 0:2]
        sc, mn = np.tile([1, 32], 4), np.tile([0, 37], 4)                # get_scale_min_k4 inverted
        q = [sc[j] | (sc[j + 4] >> 4) << 6 for j in range(4)] + [mn[j] | (mn[j + 4] >> 4) << 6 for j in range(4)]
        b[:, 4:16] = np.array(q + [(sc[j + 4] & 15) | (mn[j + 4] & 15) << 4 for j in range(4)], np.uint8)
    return b.reshape(n, -1)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_scales_far_apart(t, split):
    rng = np.random.default_rng(t)
    for k, m in ((768, 65), (512, 9)):
        run(t, rng.standard_normal((m, k)).astype(np.float32), far_apart(t, 72, k), k, m, 72, split=split)


def split_fifth_bits(t, blocks):
    """A 5-bit matrix whose fifth bits are set in elements 0 .. 15 of every run and clear in 16 .. 31 (odd rows: the other way)."""
    b = blocks.reshape(blocks.shape[0], -1, T.BLOCK[t][1])
    if t == T.Q5_K:   # qh byte l: bit 2j / 2j + 1 of element l of runs 2j / 2j + 1
        b[0::2, :, 16:32], b[0::2, :, 32:48], b[1::2, :, 16:32], b[1::2, :, 32:48] = 0xFF, 0, 0, 0xFF
    else:
        at = 2 if t == T.Q5_0 else 4
        b[0::2, :, at:at + 4], b[1::2, :, at:at + 4] = (0xFF, 0xFF, 0, 0), (0, 0, 0xFF, 0xFF)
    return b.reshape(blocks.shape)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_one_hot_rows(t, split):
    k, n = 512, 72
    at = np.sort(np.concatenate([np.arange(e, k, 32) for e in (0, 15, 16, 31)]))   # 64 rows: four elements of each of 16 runs
    a = np.zeros((64, k), np.float32)
    a[np.arange(64), at] = 1.0
    for blocks in (T.random_blocks(t, n, k, np.random.default_rng(7 * t)), far_apart(t, n, k)):
        run(t, a, blocks, k, 64, n, split=split, exact=t in EXACT)
        if t not in (T.Q4_0, T.Q4_1):
            run(t, a, split_fifth_bits(t, blocks.copy()), k, 64, n, split=split, exact=t in EXACT)


@pytest.mark.parametrize("t", TYPES, ids=TYPES.values())
def test_epilogues_and_layout(t):
    rng = np.random.default_rng(50 + t)
    m, n, k = 65, 200, 512
    a, blocks = rng.standard_normal((m, k)).astype(np.float32), T.random_blocks(t, n, k, rng)
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


# ---- whole models: the three files of test_gpu_gguf_affine, model seed 21 ------------------------------------------------------------
# name: {prompt seed: the prompts of wide_cases.prompts(seed, vocab) whose float64 greedy runs are clear at every step} -- the two best
# logits more than 100 bars apart (qwen3_ref64.assert_margins) and, with Q6_K linears, no Q8_K input within TAU of a rounding
# boundary; found on the CPU with the reference alone, clear_run() asserts both again.  Within TAU lie 4e-4 of all inputs, and the
# Q6_K linears of llama_mix read 1 536 inputs per token (qwen224: 512), so only runs of a few tokens are clear, a prompt or two per
# seed: those two models draw from several seeds.
CLEAR = {
    "qwen224": {0: (21, 23, 26), 2: (10, 11, 40), 3: (5, 13, 49, 51, 58), 4: (2, 39, 48), 5: (38, 68), 6: (30, 36), 7: (7, 18, 66)},
    "llama_mix": {2: (54,), 8: (36,), 9: (24,), 11: (22,), 14: (25,), 24: (46,), 26: (9,), 33: (19,), 45: (60,), 51: (51,), 62: (49,),
                  64: (58,), 74: (69,), 104: (16,), 108: (63,), 120: (60,), 124: (68,), 144: (26,), 146: (41,), 153: (7, 48)},
    "llama_q4_0": {0: (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 17, 18, 20, 21, 22, 23, 25, 26, 28, 30, 31)}}


def clear_run(ref, cfg, p, limit):
    """The float64 greedy ids of a prompt, its margins asserted."""
    ref.calls, ref.near, ref.flip = 0, [], frozenset()
    ids = FC.clear_greedy(ref, cfg, p, limit, "reference")
    assert not ref.near, ("a Q8_K input within TAU of a boundary", TAU, ref.near[:2])
    return ids


@pytest.fixture(scope="module", params=list(MODELS))
def model(request, tmp_path_factory):
    import kjarni_amd
    geometry, types, _, fwd_seed, _ = MODELS[request.param]
    path = str(tmp_path_factory.mktemp(request.param) / "model.gguf")
    cfg, hf = T.gguf_model(path, geometry, types, seed=21)
    clear = [(WC.prompts(seed, cfg["vocab_size"])[i], WC.max_new(seed)[i]) for seed, picks in CLEAR[request.param].items() for i in picks]
    assert len(clear) >= 16
    return kjarni_amd.HipDecoder(path), reference(hf, cfg, types), cfg, fwd_seed, clear


def test_forward_switch_on_against_float64_and_switch_off(model):
    dec, ref, cfg, seed, _ = model
    rng = np.random.default_rng(seed)                                    # test_gpu_gguf_affine's draws, in its order: the 40-token one
    for n in (5, 1, 1, 3):
        rng.integers(4, cfg["vocab_size"], n)
    ids = rng.integers(4, cfg["vocab_size"], 40).tolist()
    ref.calls, ref.near, ref.flip, cache = 0, [], frozenset(), ref.new_cache()
    raw = ref.forward(ids, cache)
    outs = {}
    for on in (False, True):
        dec.set_affine_matrix_cores(on)
        assert dec.affine_matrix_cores() is on
        dec.reset()
        h, logits = dec.forward(ids)
        outs[on] = (h, logits, [dec.kv_rows(layer) for layer in range(cfg["num_hidden_layers"])])
    dec.set_affine_matrix_cores(False)
    h, logits, kv = outs[True]
    close(h[-8:], ref.rms_norm(raw, ref.t["model.norm.weight"])[-8:])
    close(logits, logits_of(ref, raw[-1]))
    for layer in range(cfg["num_hidden_layers"]):
        for got, want, off in zip(kv[layer], cache[layer], outs[False][2][layer]):
            close(got, want)
            close(got, off)
    close(h, outs[False][0])
    close(logits, outs[False][1])


@pytest.mark.parametrize("lanes", [9, 64])
def test_generate_wide(model, lanes):
    dec, ref, cfg, _, clear = model
    reqs = [clear[i % len(clear)] for i in range(lanes + 8)]             # more requests than lanes: the lanes turn over
    want = {id(p): clear_run(ref, cfg, p, m) for p, m in clear}
    dec.set_affine_matrix_cores(True)
    got = dec.generate_wide([p for p, _ in reqs], [m for _, m in reqs], lanes=lanes, lane_context=WC.LANE_CONTEXT)
    dec.set_affine_matrix_cores(False)
    for (p, m), g in zip(reqs, got):
        assert g == want[id(p)] == dec.generate(p, m), p


def test_the_switch_off_on_off(model):
    dec, _, _, _, clear = model
    ps = [p for p, _ in clear[:9]]
    for on in (False, True, False):
        dec.set_affine_matrix_cores(on)
        dec.set_ggml_matrix_cores(True)                                  # stays a no-op on these files
        assert dec.affine_matrix_cores() is on and dec.ggml_matrix_cores() is False
        if on:
            assert len(dec.generate_wide(ps, 2, lanes=9, lane_context=WC.LANE_CONTEXT)) == 9
        else:
            with pytest.raises(Exception, match="more than 8 lanes do not take a quantized \\(GGUF\\) checkpoint: the prompt GEMM would dequantize"):
                dec.generate_wide(ps, 2, lanes=9, lane_context=WC.LANE_CONTEXT)


def test_q8_0_of_hidden_224_runs_nine_lanes(tmp_path):
    import kjarni_amd
    from tests.llm_ref64 import Ref64
    path = str(tmp_path / "model.gguf")
    cfg, hf = T.gguf_model(path, T.QWEN_224, {key: 8 for key in ALL}, seed=21)
    dec = kjarni_amd.HipDecoder(path)
    dec.set_ggml_matrix_cores(True)
    dec.set_affine_matrix_cores(True)
    assert dec.affine_matrix_cores() and not dec.ggml_matrix_cores()
    prompts, ref = WC.prompts(0, cfg["vocab_size"])[:9], Ref64(hf, cfg)
    for p, got in zip(prompts, dec.generate_wide(prompts, 6, lanes=9, lane_context=WC.LANE_CONTEXT)):
        assert len(got) == 6
        check_greedy(ref, p, got)


def test_generator_and_chat_carry_the_switch(tmp_path):
    from kjarni_amd import Chat, Generator
    from kjarni_amd.chat import GenerationConfig
    d = tmp_path / "gguf"
    T.gguf_model(str(d / "model.gguf"), dict(G.LLAMA_Q, vocab_size=720, bos_token_id=700, eos_token_id=701), {key: T.Q4_0 for key in ALL}, seed=13,
                 rope_freqs=True)
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), str(d / "tokenizer.json"))
    cfg = GenerationConfig(do_sample=False, max_new_tokens=8)
    message = "Is water wet? Answer in one short sentence, and say why you think so."      # more than 24 tokens: the prompt route
    texts = [f"{message} {i}" for i in range(12)]
    for obj, call in ((Chat("llama3.2-1b-instruct", model_path=str(d)), lambda o: o.send(message, cfg)),
                      (Generator("llama3.2-1b-instruct", model_path=str(d)), lambda o: o.generate_batch(texts, cfg))):
        plain = call(obj)
        obj.set_affine_matrix_cores(True)
        if isinstance(obj, Generator):
            obj.set_wide_lanes(16)                                       # 12 texts on the wide bank: refused with the switch off
        assert call(obj) == plain
        obj.set_affine_matrix_cores(False)
