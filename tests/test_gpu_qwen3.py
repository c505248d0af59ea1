"""Qwen3 decoders on the GPU: the per-head RMSNorm + RoPE kernel alone against float64 (kjarni_hip_op_qk_norm_rope), whole
models through every loop -- 8-row passes, single steps, the matrix-core prompt routes, the captured step, lanes,
prompt-lookup (greedy and sampled), scoring, prefix reuse, Chat -- against tests/qwen3_ref64.py, and the loader's refusals.

Bar: max |got - ref| <= 1e-4 * max(1, max |ref|) (llm_ref64.TOL), per layer and per K / V, and per logits row.  Token ids are
compared only on seeds chosen on the CPU (tests/qwen3_fixture.py) where the float64 reference's two best logits are more than
100 bars apart at every compared step; each such test asserts that margin again on what it uses."""
import json
import os
import shutil

import numpy as np
import pytest

from oracle import llm_oracle
from tests import llm_ref64 as R
from tests import lookup_cases as LK
from tests import qwen3_fixture as F
from tests import sampled_lookup_cases as S
from tests.qwen3_ref64 import Qwen3Ref64, assert_margins, log_softmax

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F64 = np.float64


def _within(got, ref, what):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), R.TOL * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _check_cache(dec, cache, what):
    assert dec.cache_len() == cache[0][0].shape[0], what
    got = [dec.kv_rows(i) for i in range(len(cache))]
    for (layer, name), (err, bar) in sorted(R.cache_errors(got, cache).items()):
        print(f"{what}: layer {layer} {name} err {err:.3e} bar {bar:.3e}")
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e} (first bad row " \
                           f"{R.first_bad_row(got[layer]['kv'.index(name)], cache[layer]['kv'.index(name)], bar)})"


def _load(tmp, geo, bf16=False, seed=F.MODEL_SEED, max_context=0, **over):
    import kjarni_amd
    d = str(tmp / f"q3-{geo['hidden_size']}-{geo['head_dim']}-{int(bf16)}-{seed}")
    cfg, t = F.qwen3_model(d, geo, seed=seed, store_bf16=bf16, **over)
    dec = kjarni_amd.HipDecoder(d, max_context=max_context)
    assert dec.bf16 == bf16 and dec.head_dim == cfg["head_dim"] and dec.hidden == cfg["hidden_size"]
    return dec, Qwen3Ref64(t, cfg), cfg


@pytest.fixture(scope="module")
def d128(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("q3_d128"), F.Q3_D128)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("q3_small"), F.Q3_SMALL)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

KERNEL_CASES = [  # head_dim, heads, kv_heads, rows, pos, pos on the device, K at its cache row
    (16, 3, 1, 1, 0, False, False), (16, 4, 2, 33, 37, True, True), (32, 3, 1, 5, 37, False, True), (32, 4, 2, 8, 0, True, False),
    (64, 3, 1, 8, 37, True, True), (64, 4, 2, 5, 0, False, False), (128, 4, 2, 33, 37, False, True), (128, 3, 1, 1, 37, True, False),
]


@pytest.mark.parametrize("d,heads,kvh,rows,pos,on_device,cache_row", KERNEL_CASES)
def test_qk_norm_rope_kernel_against_float64(d, heads, kvh, rows, pos, on_device, cache_row):
    from kjarni_amd import ops
    rng = np.random.default_rng(d * 1000 + rows)
    eps, half = 1e-6, d // 2
    ldq, ldk = heads * d + 2 * kvh * d + 7, kvh * d + 5          # (a staging row: Q | K | V and padding; a cache row and padding)
    q_rows, k_rows = rows + 2, (pos + rows + 3 if cache_row else rows + 2)
    q = (rng.standard_normal((q_rows, ldq)) * 2.0).astype(np.float32)
    k = (rng.standard_normal((k_rows, ldk)) * 0.5).astype(np.float32)
    gq, gk = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32), (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    cos, sin = llm_oracle.rope_tables(d, pos + rows + 1, 1000000.0, None)
    cos, sin = np.ascontiguousarray(cos[:, :half], np.float32), np.ascontiguousarray(sin[:, :half], np.float32)

    def ref_heads(x, n, g, p):    # x [n * d] float32 at position p
        v = x.astype(F64).reshape(n, d)
        y = v / np.sqrt((v * v).mean(-1, keepdims=True) + eps) * g.astype(F64)
        c, s = cos[p].astype(F64), sin[p].astype(F64)
        return np.concatenate([y[:, :half] * c - y[:, half:] * s, y[:, :half] * s + y[:, half:] * c], axis=-1).reshape(-1)

    want_q, want_k = q.astype(F64), k.astype(F64)
    q_mask, k_mask = np.zeros(q.shape, bool), np.zeros(k.shape, bool)
    for r in range(rows):
        kr = pos + r if cache_row else r
        want_q[r, :heads * d] = ref_heads(q[r, :heads * d], heads, gq, pos + r)
        want_k[kr, :kvh * d] = ref_heads(k[kr, :kvh * d], kvh, gk, pos + r)
        q_mask[r, :heads * d] = True
        k_mask[kr, :kvh * d] = True
    got_q, got_k = ops.qk_norm_rope(q, k, rows, heads, kvh, d, gq, gk, eps, cos, sin, pos, pos_on_device=on_device, k_at_cache_row=cache_row)
    _within(got_q[q_mask], want_q[q_mask], "q")
    _within(got_k[k_mask], want_k[k_mask], "k")
    # everything else -- padding between rows, rows past the call, other cache rows, the K | V columns of a staging row -- bit for bit
    assert np.array_equal(got_q[~q_mask].view(np.uint32), q[~q_mask].view(np.uint32))
    assert np.array_equal(got_k[~k_mask].view(np.uint32), k[~k_mask].view(np.uint32))
    assert not np.array_equal(got_q[q_mask], q[q_mask])


def test_qk_norm_rope_hook_validates():
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniException
    q, k, g = np.zeros((2, 64), np.float32), np.zeros((2, 32), np.float32), np.ones(32, np.float32)
    t = np.ones((4, 16), np.float32)
    for kw in (dict(rows=3), dict(rows=2, pos=3), dict(rows=2, pos=1, k_at_cache_row=True), dict(rows=2, n_heads=3)):
        a = dict(rows=2, n_heads=2, n_kv_heads=1, head_dim=32, pos=0) | kw
        with pytest.raises(KjarniException):
            ops.qk_norm_rope(q, k, a["rows"], a["n_heads"], a["n_kv_heads"], a["head_dim"], g, g, 1e-6, t, t, a["pos"],
                             k_at_cache_row=a.get("k_at_cache_row", False))


# ---- 2. whole models: every layer's K / V rows and the last logits ------------------------------------------------------------------

@pytest.mark.parametrize("name,bf16", [("Q3_SMALL", False), ("Q3_EVEN", False), ("Q3_D128", False), ("Q3_D128", True)])
def test_model_against_float64(tmp_path, name, bf16):
    geo = getattr(F, name)
    dec, ref, cfg = _load(tmp_path, geo, bf16)
    rng = np.random.default_rng(3)
    cache = ref.new_cache()
    for i, n in enumerate((5, 1, 1, 30, 1, 1)):      # an 8-row pass, steps, the GEMM prompt route, steps again
        ids = rng.integers(4, cfg["vocab_size"], n).tolist()
        hidden, logits = dec.forward(ids)
        h = ref.forward(ids, cache)
        _within(logits, ref.logits(h[-1:])[0], f"{name} block {i} ({n} rows): logits")
        rows = (n - 1) % 8 + 1
        _within(hidden, ref.final_norm(h[-rows:]), f"{name} block {i}: final-normed hidden rows")
    _check_cache(dec, cache, name)
    assert dec.tile_gemm_calls() == 0


def _widths_run(tmp_path, n_prompt, **over):
    dec, ref, cfg = _load(tmp_path, F.Q3_06B_WIDTHS, **over)
    rng = np.random.default_rng(4)
    cache = ref.new_cache()
    ids = rng.integers(4, cfg["vocab_size"], n_prompt).tolist()
    _, logits = dec.forward(ids)
    _within(logits, ref.logits(ref.forward(ids, cache)[-1:])[0], "prompt logits")
    tiles = dec.tile_gemm_calls()
    for i in range(4):    # one-token steps: the output projection merges the attention's slabs itself (k = q_dim = 2048)
        tok = rng.integers(4, cfg["vocab_size"], 1).tolist()
        _, logits = dec.forward(tok)
        _within(logits, ref.logits(ref.forward(tok, cache)[-1:])[0], f"step {i} logits")
    _check_cache(dec, cache, f"widths {n_prompt}")
    return tiles


def test_06b_widths_600_token_prompt_then_steps(tmp_path):
    """hidden 1024 under q_dim 2048.  At 600 rows no projection of this shape has the 208 tiles of 128 x 128 the tile route asks
    for (5 row tiles x 24 column tiles at most): the prompt runs the 64 x 64 kernel, which the counter states."""
    assert _widths_run(tmp_path, 600) == 0


def test_06b_widths_tile_prompt_route(tmp_path):
    """The 128 x 128-tile prompt route with q_dim != hidden: 1 600 rows are 13 row tiles, so the Q projection (16 column tiles)
    and gate / up (24) reach 208 tiles; K, V, o and down (8) do not.  Three tile projections per layer."""
    assert _widths_run(tmp_path, 1600, max_position_embeddings=2048) == 3 * F.Q3_06B_WIDTHS["num_hidden_layers"]


# ---- 3. one route against another ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["small", "d128"])
def test_prompt_route_equals_steps(which, request):
    dec, ref, cfg = request.getfixturevalue(which)
    ids = F.seeded_prompt(9, cfg["vocab_size"], 40)
    dec.reset()
    _, lg_a = dec.forward(ids)                        # the matrix-core route
    rows_a = [dec.kv_rows(i) for i in range(dec.layers)]
    dec.reset()
    dec.forward(ids[:5])                              # an 8-row pass, then single steps
    for t in ids[5:]:
        _, lg_b = dec.forward([t])
    _within(lg_b, lg_a, "logits")
    for i in range(dec.layers):
        kb, vb = dec.kv_rows(i)
        _within(kb, rows_a[i][0], f"layer {i} k")
        _within(vb, rows_a[i][1], f"layer {i} v")
    cache = ref.new_cache()
    _within(lg_b, ref.logits(ref.forward(ids, cache)[-1:])[0], "logits against float64")
    _check_cache(dec, cache, which)


@pytest.mark.parametrize("name", sorted(F.GREEDY_PROMPT_SEED))
def test_captured_step_generates_the_reference_ids(tmp_path, name):
    geo = getattr(F, name)
    dec, ref, cfg = _load(tmp_path, geo)
    prompt = F.seeded_prompt(F.GREEDY_PROMPT_SEED[name], cfg["vocab_size"], 9)
    want, gaps, tops = ref.greedy(prompt, 12)
    assert_margins(gaps, tops, name)
    assert cfg["eos_token_id"] not in want
    assert dec.generate(prompt, 12) == want


# ---- 4. lanes ---------------------------------------------------------------------------------------------------------------------

def test_lanes_against_float64(d128):
    dec, ref, cfg = d128
    V = cfg["vocab_size"]
    prompts = [F.seeded_prompt(seed, V, n) for n, seed in F.LANE_PROMPTS] + [F.seeded_prompt(7, V, 5)]
    before = dec.lane_gemv_calls()
    dec.lanes_begin(4, 64)
    caches = []
    for lane, p in enumerate(prompts):
        dec.lane_prefill(lane, p)
        caches.append(ref.new_cache())
        ref.forward(p, caches[-1])
    frozen = [dec.lane_kv_rows(3, i) for i in range(dec.layers)]
    rng = np.random.default_rng(12)
    for step in range(2):
        ids = rng.integers(4, V, 4).tolist()
        hidden, logits = dec.lanes_step(ids, live=[1, 1, 1, 0])
        for lane in range(3):
            h = ref.forward([ids[lane]], caches[lane])
            _within(hidden[lane], ref.final_norm(h)[0], f"step {step} lane {lane} hidden")
            _within(logits[lane], ref.logits(h)[0], f"step {step} lane {lane} logits")
    for lane in range(3):
        assert dec.lane_cache_len(lane) == len(prompts[lane]) + 2
        got = [dec.lane_kv_rows(lane, i) for i in range(dec.layers)]
        for key, (err, bar) in R.cache_errors(got, caches[lane]).items():
            assert err <= bar, (lane, key, err, bar)
    assert dec.lane_cache_len(3) == 5
    for i in range(dec.layers):      # the frozen lane: nothing written, not even at its next row
        k, v = dec.lane_kv_rows(3, i)
        assert np.array_equal(k.view(np.uint32), frozen[i][0].view(np.uint32)) and np.array_equal(v.view(np.uint32), frozen[i][1].view(np.uint32))
    streamed, fallback = (a - b for a, b in zip(dec.lane_gemv_calls(), before))
    assert streamed > 0 and fallback == 0, (streamed, fallback)        # k >= 512 everywhere: the multi-row streaming GEMV


def test_generate_batch_equals_generate(d128):
    dec, ref, cfg = d128
    prompts = [F.seeded_prompt(seed, cfg["vocab_size"], n) for n, seed in F.LANE_PROMPTS]
    want = []
    for p in prompts:
        ids, gaps, tops = ref.greedy(p, 8)
        assert_margins(gaps, tops, f"prompt of {len(p)}")
        assert cfg["eos_token_id"] not in ids
        want.append(ids)
    assert [dec.generate(p, 8) for p in prompts] == want
    assert dec.generate_batch(prompts, 8, lanes=3, lane_context=64) == want


# ---- 5. prompt-lookup ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [4, 8])
def test_verify_step_logits(d128, rows):
    dec, ref, cfg = d128
    V = cfg["vocab_size"]
    prompt = F.seeded_prompt(21, V, 13)
    block = F.seeded_prompt(22, V, 4)       # the token and a 3-token draft
    dec.reset()
    dec.forward(prompt, fetch=False)
    cache = ref.new_cache()
    ref.forward(prompt, cache)
    want = ref.logits(ref.forward(block, cache))
    picks, accepted, logits = dec.verify_step(block[0], block[1:], rows=rows)
    assert logits.shape == (4, V)
    for r in range(4):
        _within(logits[r], want[r], f"{rows}-row block, row {r}")
    assert dec.cache_len() == len(prompt) + accepted + 1
    kept = [(k[:dec.cache_len()], v[:dec.cache_len()]) for k, v in cache]
    _check_cache(dec, kept, f"verify {rows}")
    s, f = dec.verify_gemv_calls()
    assert s > 0


def test_generate_lookup_equals_generate(d128):
    dec, ref, cfg = d128
    prompt = F.lookup_prompt(F.LOOKUP_PROMPT_SEED, cfg["vocab_size"])
    want, gaps, tops = ref.greedy(prompt, 16)
    assert_margins(gaps, tops, "lookup")
    assert cfg["eos_token_id"] not in want
    assert dec.generate(prompt, 16) == want
    got, stats = dec.generate_lookup(prompt, 16)
    assert got == want
    sim = LK.simulate(prompt, want)
    # (the last simulated step's acceptance is a lower bound: the output may end inside its draft -- lookup_cases.simulate)
    body = sum(a for _, a in sim[:-1])
    assert body > 0 and body + sim[-1][1] <= stats["accepted_tokens"] <= body + sim[-1][0], (stats, sim)
    assert stats["verify_steps"] == len(sim) and stats["single_row_steps"] == 0


class _Qwen364:
    """tests/sampled_lookup_cases.py's model interface over the Qwen3 reference."""
    def __init__(self, ref, vocab):
        self.ref, self.vocab, self.first_id = ref, vocab, 4

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        return self.ref.logits(self.ref.forward(list(ids), cache))


def test_sampled_lookup_equals_the_plain_sampled_loop(d128):
    dec, ref, cfg = d128
    params = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05)
    model = _Qwen364(ref, cfg["vocab_size"])
    prompt = tr = why = None
    for seed in range(8):       # the first seeded prompt on which the float64 trace meets every precondition (asserted there)
        prompt = F.lookup_prompt(3000 + seed, cfg["vocab_size"])
        try:
            tr = S.build_trace(model, prompt, 16, params, avoid=(cfg["eos_token_id"],))
            break
        except AssertionError as e:
            why = e
    assert tr is not None, f"precondition: no seeded prompt gives a clear trace ({why})"
    kw = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05, repetition_penalty=1.0)
    plain, st0 = dec.generate_sampled(prompt, 16, lookup=None, uniforms=tr.uniforms, **kw)
    got, st = dec.generate_sampled(prompt, 16, lookup=LK.DEFAULT, uniforms=tr.uniforms, **kw)
    assert plain == tr.ids and got == plain
    assert st0 == dict.fromkeys(st0, 0) and st["verify_steps"] == len(tr.steps) and st["single_row_steps"] == 0
    assert st["accepted_tokens"] == sum(a for _, a in tr.steps) > 0


# ---- 6. scoring -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["small", "d128"])
@pytest.mark.parametrize("fused", [True, False])
def test_score_against_float64(which, fused, request):
    dec, ref, cfg = request.getfixturevalue(which)
    ids = F.seeded_prompt(31, cfg["vocab_size"], 40)
    logits = ref.logits(ref.forward(ids, ref.new_cache()))[:-1]      # row p predicts ids[p + 1]
    lsm = log_softmax(logits)
    want = lsm[np.arange(39), ids[1:]]
    bar = 2.0 * R.TOL * max(1.0, float(np.abs(logits).max()))        # tests/test_gpu_score.py: logprob = x_t - lse carries 2 B
    before = dec.score_calls()
    dec.set_score_fused(fused)
    try:
        lp, top, tlp = dec.score(ids)
    finally:
        dec.set_score_fused(True)
    f, r = (a - b for a, b in zip(dec.score_calls(), before))
    assert (f > 0 and r == 0) if fused else (f == 0 and r > 0), (f, r)
    err = float(np.abs(lp.astype(F64) - want).max())
    terr = float(np.abs(tlp.astype(F64) - lsm.max(axis=1)).max())
    print(f"{which} fused={fused}: logprob err {err:.3e} top err {terr:.3e} bar {bar:.3e}")
    assert np.isfinite(lp).all() and err <= bar and terr <= bar
    gaps = np.diff(np.partition(logits, -2, axis=1)[:, -2:], axis=1)[:, 0]
    clear = gaps > 100.0 * R.TOL * max(1.0, float(np.abs(logits).max()))
    assert (top[clear].astype(np.int64) == np.argmax(logits, axis=1)[clear]).all()


# ---- 7. prefix reuse ------------------------------------------------------------------------------------------------------------------

def test_prefix_reuse_keeps_the_shared_rows(small):
    dec, ref, cfg = small
    V = cfg["vocab_size"]
    A = F.seeded_prompt(41, V, 27)
    B = A[:20] + [t for t in F.seeded_prompt(42, V, 9) if t != A[20]][:6]
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        dec.forward(A, fetch=False)
        before = dec.prefix_stats()
        assert dec.generate(B, 0) == []
        assert tuple(a - b for a, b in zip(dec.prefix_stats(), before)) == (20, len(B) - 20)
        assert dec.resident() == B and dec.cache_len() == len(B)
        reused = dec.last_logits()
    finally:
        dec.set_prefix_reuse(False)
    dec.reset()
    _, plain = dec.forward(B)
    _within(reused, plain, "reuse against the no-reuse run")
    cache = ref.new_cache()
    _within(reused, ref.logits(ref.forward(B, cache)[-1:])[0], "reuse against float64")
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        dec.forward(A, fetch=False)
        dec.generate(B, 0)
        _check_cache(dec, cache, "reuse")
    finally:
        dec.set_prefix_reuse(False)


# ---- 8. Chat and Generator --------------------------------------------------------------------------------------------------------------

def test_chat_is_chatml_without_bos_and_replies_with_generate_ids(tmp_path):
    import kjarni_amd
    from kjarni_amd.chat import BpeTokenizer, Chat, GenerationConfig
    d = str(tmp_path / "chat")
    cfg, t = F.qwen3_model(d, F.Q3_SMALL, seed=F.CHAT_MODEL_SEED, vocab_size=720, bos_token_id=700, eos_token_id=702)
    shutil.copy(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    chat = Chat("Qwen/Qwen3-0.6B", model_path=d)
    assert chat.model_name == "qwen3-0.6b"
    r = chat.resolve()       # no generation_config.json: the Qwen2 fallback block
    assert (r.strategy, r.top_k, r.add_bos_token, r.max_new_tokens) == ("sample", 40, False, 512) and abs(r.repetition_penalty - 1.1) < 1e-6
    prompt = chat.format_prompt(None, "Hi")
    assert prompt == "<|im_start|>system\nYou are a helpful assistant.<|im_end|>\n<|im_start|>user\nHi<|im_end|>\n<|im_start|>assistant\n"
    ids = chat.encode(prompt)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    assert ids == tok.encode(prompt) and ids[0] != 700
    want, gaps, tops = Qwen3Ref64(t, cfg).greedy(ids, 10)
    assert_margins(gaps, tops, "chat")
    assert 702 not in want
    dec = kjarni_amd.HipDecoder(d)
    assert dec.generate(ids, 10) == want
    del dec
    pieces = []
    chat.stream("Hi", pieces.append, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=10))
    assert pieces == [tok.decode([i], False) for i in want]
    # the Generator accepts the same names
    from kjarni_amd import Generator
    del chat
    gen = Generator("qwen3-0.6b", model_path=d)
    assert gen.model_name == "qwen3-0.6b"
    assert gen.generate(prompt, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=10)) == "".join(pieces)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------

def _load_error(d):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniException
    with pytest.raises(KjarniException) as e:
        kjarni_amd.HipDecoder(d)
    return str(e.value)


def test_config_and_loader_refusals(tmp_path):
    import kjarni_amd
    cfg = dict(F.Q3_SMALL)
    t = F.qwen3_tensors(cfg, seed=1)
    # head_dim 32 over hidden 64 parses and loads as qwen3 ...
    dec = kjarni_amd.HipDecoder(F.write_dir(str(tmp_path / "ok"), cfg, t))
    assert (dec.head_dim, dec.hidden, dec.kv_heads) == (32, 64, 2)
    del dec
    # ... and is still refused under another model_type
    for mt in ("llama", "qwen2", "mistral"):
        assert "unsupported head geometry" in _load_error(F.write_dir(str(tmp_path / mt), dict(cfg, model_type=mt), t))
    for nm in ("q_norm", "k_norm"):
        name = f"model.layers.1.self_attn.{nm}.weight"
        msg = _load_error(F.write_dir(str(tmp_path / nm), cfg, {k: v for k, v in t.items() if k != name}))
        assert name in msg, msg
    bad = dict(t)
    bad["model.layers.0.self_attn.k_norm.weight"] = np.ones(16, np.float32)
    assert "model.layers.0.self_attn.k_norm.weight has an unexpected shape" in _load_error(F.write_dir(str(tmp_path / "shape"), cfg, bad))
