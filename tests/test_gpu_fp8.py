"""FP8 (e4m3fn) decoder checkpoints on the GPU, the codes kept in HBM: the FP8 linear kernels alone (every code exactly; the three
scale kinds against float64), whole models against oracle/llm_oracle.py and the float64 references on the dequantized f32 twin and
against the twin loaded on the existing path, every decode loop against plain generate, the weights modes and the refusals.

Bars.  The op: 1e-5 x max(1, max |ref|), the bar of test_gpu_gguf.test_linear_ggml_vs_float64 (f32 accumulation over k <= 8 192
products).  Whole models: 1e-4 against the f32 oracle (test_gpu_gguf.TOL), llm_ref64.TOL x max(1, max |ref|) against float64.
Token ids are compared under the tie rule of test_gpu_gguf._check: a difference is accepted only where the oracle's own logits
of the two tokens are within 1e-4."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from oracle import llm_oracle as LO
from tests import fp8_fixture as F
from tests import llm_ref64 as R64
from tests.qwen3_ref64 import Qwen3Ref64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu
TOL = 1e-4
F64 = np.float64


def _linear(x, codes, scale, kind):
    import kjarni_amd
    n, k = codes.shape
    x = np.ascontiguousarray(x, np.float32)
    c = np.ascontiguousarray(codes, np.uint8)
    s = np.ascontiguousarray(scale, np.float32)
    rows, cols = F.scale_shape(kind, n, k)
    y = np.empty((x.shape[0], n), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = kjarni_amd.lib().kjarni_hip_op_linear_fp8(0, fp(x), x.shape[0], c.ctypes.data_as(C.c_void_p), fp(s), rows, cols, n, k, fp(y))
    assert rc == 0, kjarni_amd._ffi.last_error()
    return y


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 8, 24], ids=["step", "rows8", "prompt"])
def test_every_code_through_the_linear_op(m):
    """Row i holds the i-th non-NaN code at column i % 128 and zeros elsewhere; x = ones; per-tensor scale 1: y is the table."""
    n, k = 254, 128
    codes = np.zeros((n, k), np.uint8)
    codes[np.arange(n), np.arange(n) % k] = F.FINITE_CODES
    y = _linear(np.ones((m, k), np.float32), codes, np.ones(1, np.float32), "tensor")
    want = F.TABLE[F.FINITE_CODES]
    for r in range(m):
        assert np.array_equal(y[r], want), (r, np.nonzero(y[r] != want)[0][:8])


@pytest.mark.parametrize("kind", F.KINDS)
def test_linear_fp8_vs_float64(kind):
    rng = np.random.default_rng(F.KINDS.index(kind))
    n = 200  # not a multiple of the 128-row scale block, of the columns per wave or per workgroup
    for k in (128, 384, 2048, 8192):  # below one K-slice of the kernel, an odd number of pieces, one slice exactly, four slices
        codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
        w = F.TABLE[codes].astype(F64) * F.expand_scale(scale, kind, n, k).astype(F64)
        for m in (1, 3, 8, 24, 300):
            x = rng.standard_normal((m, k)).astype(np.float32)
            ref = x.astype(F64) @ w.T
            got = _linear(x, codes, scale, kind)
            err, bar = np.abs(got - ref).max(), 1e-5 * max(1.0, np.abs(ref).max())
            print(f"{kind} k={k} m={m}: err {err:.3e} bar {bar:.3e}")
            assert np.isfinite(got).all() and err <= bar, (kind, k, m, err, bar)


def test_linear_fp8_refuses_bad_arguments():
    import kjarni_amd
    L = kjarni_amd.lib()
    x, y = np.ones((1, 32), np.float32), np.zeros((1, 4), np.float32)
    s = np.ones(8, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ok = np.zeros((4, 32), np.uint8)
    nan = ok.copy()
    nan[2, 3] = 0xFF
    for codes, rows, cols, n, k in ((ok, 2, 1, 4, 32), (ok, 1, 1, 4, 24), (nan, 1, 1, 4, 32), (ok, 4, 2, 4, 32)):
        rc = L.kjarni_hip_op_linear_fp8(0, fp(x), 1, codes.ctypes.data_as(C.c_void_p), fp(s), rows, cols, n, k, fp(y))
        assert rc != 0


# ---- 2. whole models ------------------------------------------------------------------------------------------------------------

MODELS = {  # name: (geometry, scale kind, seed)
    "llama-channel": (F.LLAMA_F8, "channel", 3),
    "qwen2-tensor": (F.QWEN2_F8, "tensor", 9),
    "llama-block": (F.LLAMA_F8, "block", 5),
    "qwen3-block": (F.QWEN3_F8, "block", 7),
}


def _load(path, weights="auto"):
    import kjarni_amd
    return kjarni_amd.HipDecoder(path, weights=weights)


class _Model:
    def __init__(self, tmp, name):
        geo, kind, seed = MODELS[name]
        self.dir, self.twin_dir = str(tmp / "fp8"), str(tmp / "twin")
        self.cfg, self.hf = F.fp8_model(self.dir, geo, kind, seed=seed, twin=self.twin_dir)
        self.qwen3 = geo["model_type"] == "qwen3"
        self.dec = _load(self.dir)
        self.ref64 = (Qwen3Ref64 if self.qwen3 else R64.Ref64)(self.hf, self.cfg)
        self.orc = None if self.qwen3 else LO.LlmOracle(self.hf, self.cfg)   # (the f32 oracle has no Qwen3 head norm)
        self._twin = None

    @property
    def twin(self):
        if self._twin is None:
            self._twin = _load(self.twin_dir)
        return self._twin

    def ref_logits64(self, h_rows):
        """float64 logits of the reference's last-layer rows."""
        head = self.ref64.t.get("lm_head.weight", self.ref64.t["model.embed_tokens.weight"])
        return self.ref64.rms_norm(h_rows, self.ref64.t["model.norm.weight"]) @ head.T

    def greedy(self, prompt, n):
        """(ids, per step the reference logits): the f32 oracle's trace, for Qwen3 the float64 reference's."""
        if self.orc is not None:
            return self.orc.generate(prompt, n, return_logits=True)
        cache = self.ref64.new_cache()
        lg = self.ref_logits64(self.ref64.forward(prompt, cache)[-1:])[0]
        ids, trace = [], []
        for _ in range(n):
            trace.append(lg)
            ids.append(int(np.argmax(lg)))
            lg = self.ref_logits64(self.ref64.forward([ids[-1]], cache)[-1:])[0]
        return ids, trace


@pytest.fixture(scope="module", params=sorted(MODELS))
def model(request, tmp_path_factory):
    return _Model(tmp_path_factory.mktemp(request.param.replace("-", "_")), request.param)


@pytest.fixture(scope="module")
def llama(tmp_path_factory):
    return _Model(tmp_path_factory.mktemp("routes_llama"), "llama-channel")


@pytest.fixture(scope="module")
def qwen3(tmp_path_factory):
    return _Model(tmp_path_factory.mktemp("routes_qwen3"), "qwen3-block")


def _check(got, exp, trace):
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:  # only where the reference's own two best logits tie within noise
            assert abs(trace[i][a] - trace[i][b]) < 1e-4, (i, a, b)
            return
    assert len(got) == len(exp)


def _within64(got, ref, what):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), R64.TOL * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def test_model_layout_and_bytes(model):
    dec, cfg = model.dec, model.cfg
    H, L, I, V = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["intermediate_size"], cfg["vocab_size"]
    qd, kv = cfg["num_attention_heads"] * cfg["head_dim"], cfg["num_key_value_heads"] * cfg["head_dim"]
    assert dec.config["model_type"] == cfg["model_type"] and dec.head_dim == cfg["head_dim"] and dec.bf16
    by = dec.weight_bytes_by_type()
    assert by["F8_E4M3"] == L * (qd * H + 2 * kv * H + H * qd + 3 * I * H)          # one byte per layer weight
    assert by["BF16"] == (1 if cfg["tie_word_embeddings"] else 2) * V * H * 2       # the table and the head, nothing else
    assert not set(by) - {"F8_E4M3", "BF16", "F32"} and sum(by.values()) == dec.weight_bytes


def test_model_vs_oracle_and_float64(model):
    dec, cfg = model.dec, model.cfg
    rng = np.random.default_rng(0)
    blocks = []
    dec.reset()
    cache64 = model.ref64.new_cache()
    cache = model.orc.new_cache() if model.orc else None
    for n in (5, 1, 1, 11, 1, 3, 1, 30, 1):      # 8-row passes, single steps (the captured kernels' shapes), the prompt route
        ids = rng.integers(4, cfg["vocab_size"], n).tolist()
        blocks.append(ids)
        h, logits = dec.forward(ids)
        k = (n - 1) % 8 + 1
        h64 = model.ref64.forward(ids, cache64)
        if model.orc:
            ref_h = model.orc.forward(ids, cache)[0]
            assert np.abs(h[-k:] - ref_h[-k:]).max() < TOL
            assert np.abs(logits - model.orc.logits(ref_h[-1])).max() < TOL
        else:
            _within64(h[-k:], model.ref64.final_norm(h64[-k:]), f"{n} rows: hidden")
        _within64(logits, model.ref_logits64(h64[-1:])[0], f"{n} rows: logits")
    # every KV row of every layer against float64 (written by 8-row passes, steps and the prompt route)
    for layer in range(cfg["num_hidden_layers"]):
        for got, want in zip(dec.kv_rows(layer), cache64[layer]):
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= R64.TOL * max(1.0, np.abs(want).max()), layer
    # a near-full prompt: far positions, the prompt route
    dec.reset()
    ids = rng.integers(4, cfg["vocab_size"], cfg["max_position_embeddings"] - 2).tolist()
    h, logits = dec.forward(ids)
    cache64 = model.ref64.new_cache()
    h64 = model.ref64.forward(ids, cache64)
    _within64(logits, model.ref_logits64(h64[-1:])[0], "near-full prompt: logits")
    if model.orc:
        ref_h = model.orc.forward(ids, model.orc.new_cache())[0]
        assert np.abs(h[-1] - ref_h[-1]).max() < TOL and np.abs(logits - model.orc.logits(ref_h[-1])).max() < TOL
    for layer in range(cfg["num_hidden_layers"]):
        for got, want in zip(dec.kv_rows(layer), cache64[layer]):
            assert np.abs(got - want).max() <= R64.TOL * max(1.0, np.abs(want).max()), layer


def test_model_vs_twin_on_the_existing_path(model):
    dec, tw, cfg = model.dec, model.twin, model.cfg
    assert "F8_E4M3" not in tw.weight_bytes_by_type()
    ids = np.random.default_rng(1).integers(4, cfg["vocab_size"], 40).tolist()
    for blocks in ([ids[:5], ids[5:6], ids[6:13]], [ids]):      # decode passes; the prompt route
        dec.reset()
        tw.reset()
        for b in blocks:
            _, la = dec.forward(b)
            _, lb = tw.forward(b)
        assert np.abs(la - lb).max() < 1e-5 * max(1.0, np.abs(lb).max())
        for layer in range(cfg["num_hidden_layers"]):
            ka, va = dec.kv_rows(layer)
            kb, vb = tw.kv_rows(layer)
            assert np.abs(ka - kb).max() < 1e-5 * max(1.0, np.abs(kb).max()) and np.abs(va - vb).max() < 1e-5 * max(1.0, np.abs(vb).max())


def test_greedy_generate_vs_reference(model):
    prompt = [1, 17, 44, 203, 9, 9, 250, 31, 77, 5, 120]
    exp, trace = model.greedy(prompt, 30)
    _check(model.dec.generate(prompt, 30), exp, trace)


# ---- 3. the routes: each loop against plain generate on the same checkpoint -----------------------------------------------------

def _lookup_prompt(seed, vocab):
    rng = np.random.default_rng(seed)
    a = rng.integers(4, vocab, 5).tolist()
    return a + a[:4] + rng.integers(4, vocab, 2).tolist() + a[:2]


@pytest.mark.parametrize("which", ["llama", "qwen3"])
def test_verify_step_against_the_reference(which, request):
    m = request.getfixturevalue(which)
    dec, V = m.dec, m.cfg["vocab_size"]
    rng = np.random.default_rng(21)
    prompt, block = rng.integers(4, V, 13).tolist(), rng.integers(4, V, 4).tolist()      # the token and a 3-token draft
    for rows in (4, 8):
        dec.reset()
        dec.forward(prompt, fetch=False)
        picks, accepted, logits = dec.verify_step(block[0], block[1:], rows=rows)
        assert logits.shape == (4, V) and dec.cache_len() == len(prompt) + accepted + 1
        cache64 = m.ref64.new_cache()
        m.ref64.forward(prompt, cache64)
        want = m.ref_logits64(m.ref64.forward(block, cache64))
        for r in range(4):
            _within64(logits[r], want[r], f"{which} {rows}-row block, row {r}")
        if m.orc:
            cache = m.orc.new_cache()
            m.orc.forward(prompt, cache)
            hs = m.orc.forward(block, cache)[0]
            for r in range(4):
                assert np.abs(logits[r] - m.orc.logits(hs[r])).max() < TOL
        n = dec.cache_len()
        for layer in range(dec.layers):
            for got, w in zip(dec.kv_rows(layer), cache64[layer]):
                assert np.abs(got - w[:n]).max() <= R64.TOL * max(1.0, np.abs(w[:n]).max())


@pytest.mark.parametrize("which", ["llama", "qwen3"])
def test_lanes_step_against_the_reference(which, request):
    m = request.getfixturevalue(which)
    dec, V = m.dec, m.cfg["vocab_size"]
    rng = np.random.default_rng(12)
    prompts = [rng.integers(4, V, n).tolist() for n in (3, 11, 26)]
    dec.lanes_begin(3, 64)
    caches = []
    for lane, p in enumerate(prompts):
        dec.lane_prefill(lane, p)
        caches.append(m.ref64.new_cache())
        m.ref64.forward(p, caches[-1])
    for step in range(2):
        ids = rng.integers(4, V, 3).tolist()
        hidden, logits = dec.lanes_step(ids)
        for lane in range(3):
            h = m.ref64.forward([ids[lane]], caches[lane])
            _within64(hidden[lane], m.ref64.rms_norm(h, m.ref64.t["model.norm.weight"])[0], f"{which} step {step} lane {lane} hidden")
            _within64(logits[lane], m.ref_logits64(h)[0], f"{which} step {step} lane {lane} logits")
    for lane in range(3):
        assert dec.lane_cache_len(lane) == len(prompts[lane]) + 2
        got = [dec.lane_kv_rows(lane, i) for i in range(dec.layers)]
        for key, (err, bar) in R64.cache_errors(got, caches[lane]).items():
            assert err <= bar, (lane, key, err, bar)


@pytest.mark.parametrize("which", ["llama", "qwen3"])
def test_loops_equal_plain_generate(which, request):
    m = request.getfixturevalue(which)
    dec, V = m.dec, m.cfg["vocab_size"]
    # prompt-lookup
    prompt = _lookup_prompt(1001, V)
    exp, trace = m.greedy(prompt, 16)
    plain = dec.generate(prompt, 16)
    _check(plain, exp, trace)
    got, stats = dec.generate_lookup(prompt, 16)
    _check(got, plain, trace)
    assert stats["verify_steps"] > 0
    # lanes: 3 requests on 2 lanes
    rng = np.random.default_rng(2000)
    prompts = [rng.integers(4, V, n).tolist() for n in (3, 11, 26)]
    batch = dec.generate_batch(prompts, 8, lanes=2, lane_context=64)
    for p, b in zip(prompts, batch):
        _check(b, dec.generate(p, 8), m.greedy(p, 8)[1])
    # a draft model: the f32 twin proposes, every emitted token is the FP8 model's own decision
    got, stats = dec.generate_draft(m.twin, prompt, 16, draft_tokens=4)
    _check(got, plain, trace)
    assert stats["verify_steps"] > 0 and stats["accepted_tokens"] > 0
    # sampled generation that can only take the best token; scoring
    got, _ = dec.generate_sampled(prompt, 16, lookup=None, top_k=1)
    _check(got, plain, trace)
    ids = prompt + plain
    lp, top, tlp = dec.score(ids)
    cache64 = m.ref64.new_cache()
    lg = m.ref_logits64(m.ref64.forward(ids, cache64))[:-1]
    mx = lg.max(axis=-1, keepdims=True)
    lsm = lg - mx - np.log(np.exp(lg - mx).sum(axis=-1, keepdims=True))
    want = lsm[np.arange(len(ids) - 1), ids[1:]]
    assert np.abs(lp.astype(F64) - want).max() <= 2.0 * R64.TOL * max(1.0, float(np.abs(lg).max()))
    # prefix reuse: the shared rows stay, the logits are those of a fresh run
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        dec.forward(prompt + plain[:6], fetch=False)
        assert dec.generate(prompt + plain[:3] + [7], 0) == []
        reused = dec.last_logits()
    finally:
        dec.set_prefix_reuse(False)
    dec.reset()
    _, fresh = dec.forward(prompt + plain[:3] + [7])
    assert np.abs(reused - fresh).max() <= R64.TOL * max(1.0, np.abs(fresh).max())


# ---- 4. weights modes, the packed entry points, refusals, Generator -------------------------------------------------------------

def test_weights_modes_agree_with_the_twin(llama):
    cfg = llama.cfg
    ids = np.random.default_rng(4).integers(4, cfg["vocab_size"], 13).tolist()
    for mode in ("f32", "bf16"):
        a, b = _load(llama.dir, weights=mode), _load(llama.twin_dir, weights=mode)
        by = a.weight_bytes_by_type()
        assert "F8_E4M3" not in by and a.bf16 == (mode == "bf16") and by == b.weight_bytes_by_type()
        for blocks in ([ids[:5], ids[5:6]], [ids + ids + ids]):
            a.reset()
            b.reset()
            for blk in blocks:
                _, la = a.forward(blk)
                _, lb = b.forward(blk)
            assert np.array_equal(la, lb)      # the same numbers in HBM, the same kernels


def test_packed_entry_points_keep_refusing(llama):
    from kjarni_amd._ffi import KjarniException
    dec = llama.dec
    seqs = [[5, 6, 7, 8], [9, 10, 11]]
    for call in (lambda: dec.embed(seqs), lambda: dec.score_batch(seqs, [1, 1]), lambda: dec.answer_logits(seqs, [4, 5])):
        with pytest.raises(KjarniException) as e:
            call()
        assert "quantized" in str(e.value)


def _load_error(path, weights="auto"):
    from kjarni_amd._ffi import KjarniException
    with pytest.raises(KjarniException) as e:
        _load(path, weights)
    return str(e.value)


def _rewrite(src, dst, edit, cfg_edit=None):
    """A copy of the FP8 directory `src` with its tensor dict passed through edit(entries)."""
    import json
    import struct
    with open(os.path.join(src, "model.safetensors"), "rb") as f:
        raw = f.read()
    hlen = struct.unpack("<Q", raw[:8])[0]
    header = json.loads(raw[8:8 + hlen])
    data = raw[8 + hlen:]
    t = {k: (v["dtype"], tuple(v["shape"]), data[v["data_offsets"][0]:v["data_offsets"][1]]) for k, v in header.items() if k != "__metadata__"}
    edit(t)
    with open(os.path.join(src, "config.json")) as f:
        cfg = json.load(f)
    if cfg_edit:
        cfg_edit(cfg)
    return F.write_dir(dst, cfg, t)


def test_load_refusals_on_the_device_path(llama, tmp_path):
    q, up = "model.layers.1.self_attn.q_proj.weight", "model.layers.0.mlp.up_proj.weight"
    n, k = llama.hf[q].shape

    def mixed(t):
        t[q] = F.entry(llama.hf[q])
        del t[q + "_scale"]
    d = _rewrite(llama.dir, str(tmp_path / "mixed"), mixed)
    msg = _load_error(d)
    assert q in msg and "F32" in msg and "weights_dtype 1 or 2" in msg
    f = _load(d, weights="f32")      # ... and 1 loads the file: the numbers of the twin
    ids = [5, 9, 200, 31, 7]
    _, la = f.forward(ids)
    llama.twin.reset()
    _, lb = llama.twin.forward(ids)
    assert np.array_equal(la, lb)
    del f

    def no_scale(t):
        del t[up + "_scale"]
    assert up in _load_error(_rewrite(llama.dir, str(tmp_path / "noscale"), no_scale))

    def both(t):
        t[up + "_scale_inv"] = t[up + "_scale"]
    msg = _load_error(_rewrite(llama.dir, str(tmp_path / "both"), both))
    assert up in msg and "both" in msg

    def shape(t):
        t[up + "_scale"] = F.entry(np.ones((7, 1), np.float32))
    msg = _load_error(_rewrite(llama.dir, str(tmp_path / "shape"), shape))
    assert up in msg and "[7, 1]" in msg

    def nan(t):
        dt, shp, raw = t[up]
        b = bytearray(raw)
        b[5 * shp[1] + 3] = 0x7F
        t[up] = (dt, shp, bytes(b))
    msg = _load_error(_rewrite(llama.dir, str(tmp_path / "nan"), nan))
    assert up in msg and "NaN" in msg
    assert up in _load_error(str(tmp_path / "nan"), "f32")      # the checker modes read through the same refusals

    msg = _load_error(_rewrite(llama.dir, str(tmp_path / "fmt"), lambda t: None, lambda c: c["quantization_config"].update(fmt="e5m2")))
    assert "e5m2" in msg and "model.layers.0" in msg
    msg = _load_error(_rewrite(llama.dir, str(tmp_path / "bs"), lambda t: None,
                               lambda c: c["quantization_config"].update(weight_block_size=[64, 64])))
    assert "[64, 64]" in msg and "model.layers.0" in msg


def test_generator_on_an_fp8_directory(tmp_path):
    import kjarni_amd
    from kjarni_amd import Generator
    from kjarni_amd.chat import BpeTokenizer, GenerationConfig
    d = str(tmp_path / "gen")
    geo = dict(F.QWEN3_F8, vocab_size=720, bos_token_id=700, eos_token_id=702)
    cfg, hf = F.fp8_model(d, geo, "block", seed=11)
    shutil.copy(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    text = "Hello there, how are you?"
    greedy = GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=12)
    gen = Generator("qwen3-0.6b", model_path=d)
    ids = gen.encode(text, greedy)
    assert ids == tok.encode(text)
    dec = kjarni_amd.HipDecoder(d)
    assert dec.weight_bytes_by_type().get("F8_E4M3", 0) > 0
    want = dec.generate(ids, 12)
    ref = Qwen3Ref64(hf, cfg)
    cache = ref.new_cache()
    lg = ref.logits(ref.forward(ids, cache)[-1:])[0]
    for i, t in enumerate(want):      # the FP8 decoder's ids are the float64 reference's, under the tie rule
        best = int(np.argmax(lg))
        if t != best:
            assert lg[best] - lg[t] < 1e-4, (i, t, best)
            break
        lg = ref.logits(ref.forward([t], cache)[-1:])[0]
    del dec
    out = gen.generate(text, greedy)
    stop = want.index(702) if 702 in want else len(want)
    assert out == "".join(tok.decode([i], False) for i in want[:stop]) and len(want) > 0
