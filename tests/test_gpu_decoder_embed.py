"""Decoder embedders on the GPU: the packed causal attention, the per-row RoPE kernels and the last-token pool alone, whole
models through HipDecoder.embed against the float64 references (tests/llm_ref64.py, tests/qwen3_ref64.py), chunking, the tile
route, what an embed call must leave untouched, validation, and the Embedder C ABI on a decoder directory.

Bar: max |got - ref| <= 1e-4 * max(1, max |ref|) (llm_ref64.TOL), against float64 restatements, never against the code under
test.  Bit-for-bit comparisons are between two runs of the same kernels, or say which existing kernel they follow."""
import json
import os

import numpy as np
import pytest

from oracle import llm_oracle
from tests import gguf_fixture as GG
from tests import gpt2_fixture as G2
from tests import llm_ref64 as R
from tests import qwen3_fixture as F
from tests import synth
from tests.qwen3_ref64 import Qwen3Ref64

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F64 = np.float64


def _within(got, ref, what):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), R.TOL * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _l2(x):
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return np.where(n > 0, x / np.where(n > 0, n, 1.0), x)


# ---- 1. attention alone ---------------------------------------------------------------------------------------------------------

CANARY = np.float32(-777.25)
LENGTH_SETS = [[1], [1, 1, 1], [31, 32, 33], [64, 65, 1, 127], [200, 7]]
MFMA_SETS = [[257, 3, 300], [256, 128]]
ATT_CASES = [(d, g, ls) for d in (16, 32, 64, 128) for g in (1, 2, 4) for ls in LENGTH_SETS + (MFMA_SETS if d >= 64 else [])]


def _att_inputs(d, group, lengths, seed):
    kvh, heads = 2, 2 * group
    rng = np.random.default_rng(seed)
    T = sum(lengths)
    rows = T + 3
    ldq, ldk, ldv, ldc = heads * d + 8, kvh * d + 4, kvh * d + 12, heads * d + 4
    q = rng.standard_normal((rows, ldq)).astype(np.float32)
    k = rng.standard_normal((rows, ldk)).astype(np.float32)
    v = rng.standard_normal((rows, ldv)).astype(np.float32)
    ctx = np.full((rows, ldc), CANARY, np.float32)
    return heads, kvh, T, q, k, v, ctx


def _att_ref(q, k, v, lengths, heads, kvh, d):
    """float64 [T, heads * d]: every sequence on its own, causal."""
    out = np.zeros((sum(lengths), heads * d), F64)
    at = 0
    for n in lengths:
        mask = np.tril(np.ones((n, n), bool))
        for h in range(heads):
            g = h // (heads // kvh)
            qh = q[at:at + n, h * d:(h + 1) * d].astype(F64)
            kh, vh = k[at:at + n, g * d:(g + 1) * d].astype(F64), v[at:at + n, g * d:(g + 1) * d].astype(F64)
            s = np.where(mask, qh @ kh.T / np.sqrt(d), -np.inf)
            p = np.exp(s - s.max(-1, keepdims=True))
            out[at:at + n, h * d:(h + 1) * d] = (p / p.sum(-1, keepdims=True)) @ vh
        at += n
    return out


@pytest.mark.parametrize("d,group,lengths", ATT_CASES, ids=lambda x: "-".join(map(str, x)) if isinstance(x, list) else str(x))
def test_packed_attention_against_float64(d, group, lengths):
    from kjarni_amd import ops
    heads, kvh, T, q, k, v, ctx = _att_inputs(d, group, lengths, d * 100 + group * 10 + len(lengths))
    got = ops.packed_causal_attention(q, k, v, lengths, heads, kvh, d, ctx=ctx)
    _within(got[:T, :heads * d], _att_ref(q, k, v, lengths, heads, kvh, d), f"d {d} group {group} lengths {lengths}")
    # rows at or past T and the padding columns: bit for bit what they were
    assert np.array_equal(_bits(got[T:]), _bits(ctx[T:])) and np.array_equal(_bits(got[:, heads * d:]), _bits(ctx[:, heads * d:]))


@pytest.mark.parametrize("d,lengths", [(32, [31, 32, 33]), (64, [31, 32, 33]), (64, [257, 3, 300]), (128, [257, 3, 300])],
                         ids=lambda x: "-".join(map(str, x)) if isinstance(x, list) else str(x))
def test_packed_attention_never_reads_another_sequence(d, lengths):
    """Everything outside sequence i -- the Q, K and V rows of the other sequences and the rows past T -- set to NaN: the rows
    of i come out bit for bit as in the clean run."""
    from kjarni_amd import ops
    heads, kvh, T, q, k, v, ctx = _att_inputs(d, 2, lengths, 7 + d)
    clean = ops.packed_causal_attention(q, k, v, lengths, heads, kvh, d, ctx=ctx)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for i, n in enumerate(lengths):
        lo, hi = int(starts[i]), int(starts[i + 1])
        qn, kn, vn = (np.full_like(x, np.nan) for x in (q, k, v))
        for dst, src in ((qn, q), (kn, k), (vn, v)):
            dst[lo:hi] = src[lo:hi]
        got = ops.packed_causal_attention(qn, kn, vn, lengths, heads, kvh, d, ctx=ctx)
        assert np.isfinite(got[lo:hi]).all(), f"sequence {i}: NaN leaked in"
        assert np.array_equal(_bits(got[lo:hi]), _bits(clean[lo:hi])), f"sequence {i} changed with its neighbours"


def test_packed_attention_hook_validates():
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniException
    q, kv = np.zeros((8, 64), np.float32), np.zeros((8, 32), np.float32)
    ok = dict(lengths=[3, 5], heads=2, kv_heads=1, head_dim=32)
    ops.packed_causal_attention(q, kv, kv, **ok)
    for kw in (dict(lengths=[3, 6]), dict(lengths=[3, 0, 5]), dict(head_dim=24), dict(heads=3, kv_heads=2), dict(heads=4)):
        with pytest.raises(KjarniException):
            ops.packed_causal_attention(q, kv, kv, **(ok | kw))
    with pytest.raises(KjarniException):      # a leading dimension that is no multiple of 4
        ops.packed_causal_attention(np.zeros((8, 66), np.float32), kv, kv, **ok)


# ---- 2. the two RoPE kernels: bit-identical, sequence by sequence, to the kernels at pos = 0 --------------------------------------

ROPE_LENGTHS = [1, 5, 33]


def _row_pos(lengths):
    return np.concatenate([np.arange(n) for n in lengths]).astype(np.int32)


@pytest.mark.parametrize("d,heads", [(16, 4), (64, 3), (128, 2)])
def test_rope_rows_equals_rope_per_sequence(d, heads):
    from kjarni_amd import ops
    rng = np.random.default_rng(d)
    T, half = sum(ROPE_LENGTHS), d // 2
    x = rng.standard_normal((T + 2, heads * d + 5)).astype(np.float32)
    cos, sin = llm_oracle.rope_tables(d, 40, 500000.0, None)
    cos, sin = np.ascontiguousarray(cos[:, :half], np.float32), np.ascontiguousarray(sin[:, :half], np.float32)
    got = ops.rope_rows(x, _row_pos(ROPE_LENGTHS), heads, d, cos, sin)
    at = 0
    for n in ROPE_LENGTHS:
        want = ops.rope(x[at:at + n], n, heads, d, cos, sin, 0)
        assert np.array_equal(_bits(got[at:at + n]), _bits(want)), f"sequence of {n} rows"
        # and the existing kernel is what float64 says
        xs = x[at:at + n, :heads * d].astype(F64).reshape(n, heads, d)
        c, s = cos[:n].astype(F64)[:, None], sin[:n].astype(F64)[:, None]
        ref = np.concatenate([xs[..., :half] * c - xs[..., half:] * s, xs[..., :half] * s + xs[..., half:] * c], -1).reshape(n, -1)
        _within(got[at:at + n, :heads * d], ref, f"rope rows of a {n}-row sequence")
        at += n
    assert np.array_equal(_bits(got[T:]), _bits(x[T:])) and np.array_equal(_bits(got[:, heads * d:]), _bits(x[:, heads * d:]))
    assert not np.array_equal(got[1:T, :heads * d], x[1:T, :heads * d])


@pytest.mark.parametrize("d,heads,kvh", [(16, 4, 2), (32, 3, 1), (128, 4, 2)])
def test_qk_norm_rope_rows_equals_qk_norm_rope_per_sequence(d, heads, kvh):
    from kjarni_amd import ops
    rng = np.random.default_rng(d + 1)
    T, half, eps = sum(ROPE_LENGTHS), d // 2, 1e-6
    q = (rng.standard_normal((T + 2, heads * d + 7)) * 2.0).astype(np.float32)
    k = (rng.standard_normal((T + 3, kvh * d + 5)) * 0.5).astype(np.float32)
    gq, gk = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32), (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    cos, sin = llm_oracle.rope_tables(d, 40, 1000000.0, None)
    cos, sin = np.ascontiguousarray(cos[:, :half], np.float32), np.ascontiguousarray(sin[:, :half], np.float32)
    got_q, got_k = ops.qk_norm_rope_rows(q, k, _row_pos(ROPE_LENGTHS), heads, kvh, d, gq, gk, eps, cos, sin)
    at = 0
    for n in ROPE_LENGTHS:
        want_q, want_k = ops.qk_norm_rope(q[at:at + n], k[at:at + n], n, heads, kvh, d, gq, gk, eps, cos, sin, 0)
        assert np.array_equal(_bits(got_q[at:at + n]), _bits(want_q)) and np.array_equal(_bits(got_k[at:at + n]), _bits(want_k)), n
        at += n
    for got, src, w in ((got_q, q, heads * d), (got_k, k, kvh * d)):      # rows outside the call and the padding: untouched
        assert np.array_equal(_bits(got[T:]), _bits(src[T:])) and np.array_equal(_bits(got[:, w:]), _bits(src[:, w:]))
        assert not np.array_equal(got[:T, :w], src[:T, :w])


def test_rope_hooks_validate_positions():
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniException
    x, t, g = np.zeros((4, 32), np.float32), np.ones((4, 8), np.float32), np.ones(16, np.float32)
    ops.rope_rows(x, [0, 3, 1], 2, 16, t, t)
    for pos in ([0, 4], [-1], [0, 1, 2, 3, 0]):
        with pytest.raises(KjarniException):
            ops.rope_rows(x, pos, 2, 16, t, t)
        with pytest.raises(KjarniException):
            ops.qk_norm_rope_rows(x, x, pos, 2, 2, 16, g, g, 1e-6, t, t)
    with pytest.raises(KjarniException):
        ops.rope(x, 3, 2, 16, t, t, 2)


# ---- 3. the pool alone --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [100, 384, 1024])
@pytest.mark.parametrize("normalize", [False, True])
def test_last_token_pool_against_float64(hidden, normalize):
    from kjarni_amd import ops
    lengths, eps = [1, 8, 3], 1e-6
    rng = np.random.default_rng(hidden)
    x = (rng.standard_normal((sum(lengths) + 2, hidden + 3)) * 3.0).astype(np.float32)
    x[8, :] = 0.0                                     # the second sequence's last row: all zeros -> zeros, with or without L2
    gamma = (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)
    got = ops.last_token_pool(x, lengths, gamma, eps, normalize)
    rows = x[[0, 8, 11], :hidden].astype(F64)
    ref = rows / np.sqrt((rows * rows).mean(-1, keepdims=True) + eps) * gamma.astype(F64)
    if normalize:
        ref = _l2(ref)
    _within(got, ref, f"pool hidden {hidden} normalize {normalize}")
    assert np.array_equal(got[1], np.zeros(hidden, np.float32))
    if normalize:
        assert np.abs(np.linalg.norm(got[[0, 2]].astype(F64), axis=-1) - 1.0).max() < 1e-5


# ---- 4. whole models ----------------------------------------------------------------------------------------------------------------

BATCH = [5, 1, 30, 9, 64]


def _make(tmp, kind, bf16=False):
    import kjarni_amd
    d = str(tmp / f"{kind}-{int(bf16)}")
    if kind in ("llama", "qwen2"):
        cfg, t = synth.llm_model(d, synth.LLAMA_TEST if kind == "llama" else synth.QWEN_TEST, seed=3)
        ref = R.Ref64(t, cfg)
        final = lambda h: ref.rms_norm(h, ref.t["model.norm.weight"])  # noqa: E731
    else:
        cfg, t = F.qwen3_model(d, getattr(F, kind), seed=F.MODEL_SEED, store_bf16=bf16)
        ref = Qwen3Ref64(t, cfg)
        final = ref.final_norm
    dec = kjarni_amd.HipDecoder(d)
    assert dec.bf16 == bf16

    def embed_ref(seqs, normalize):
        rows = np.stack([final(ref.forward(s, ref.new_cache())[-1:])[0] for s in seqs])
        return _l2(rows) if normalize else rows
    return dec, cfg, embed_ref


MODELS = [("llama", False), ("qwen2", False), ("Q3_SMALL", False), ("Q3_EVEN", False), ("Q3_D128", False), ("Q3_D128", True)]


@pytest.mark.parametrize("kind,bf16", MODELS, ids=[f"{k}{'-bf16' if b else ''}" for k, b in MODELS])
def test_embed_against_float64(tmp_path, kind, bf16):
    dec, cfg, embed_ref = _make(tmp_path, kind, bf16)
    rng = np.random.default_rng(5)
    seqs = [rng.integers(4, cfg["vocab_size"], n).tolist() for n in BATCH]
    for normalize in (True, False):
        ref = embed_ref(seqs, normalize)
        got = dec.embed(seqs, normalize)
        assert got.shape == (len(BATCH), cfg["hidden_size"])
        for i, n in enumerate(BATCH):
            _within(got[i], ref[i], f"{kind} normalize {normalize} sequence {i} ({n} tokens)")
        if normalize:
            assert np.abs(np.linalg.norm(got.astype(F64), axis=-1) - 1.0).max() < 1e-5
        for i, s in enumerate(seqs):
            # the single-sequence route the parent commit offers: forward() + last_hidden()
            dec.reset()
            hidden, _ = dec.forward(s)
            alone = hidden[-1].astype(F64)
            _within(got[i], _l2(alone) if normalize else alone, f"{kind} sequence {i} against forward() + last_hidden()")
            # and the sequence embedded on its own
            _within(dec.embed([s], normalize)[0], got[i], f"{kind} sequence {i} alone against its row of the batch")
    assert dec.tile_gemm_calls() == 0


# ---- 5. chunks and the tile route ---------------------------------------------------------------------------------------------------

def test_embed_more_rows_than_a_chunk(tmp_path):
    from kjarni_amd import embed_plan
    dec, cfg, embed_ref = _make(tmp_path, "llama")
    rng = np.random.default_rng(17)
    lengths = rng.integers(60, 121, 40).tolist()
    assert sum(lengths) > 2048
    first, vec, mfma = embed_plan(lengths, dec.head_dim)
    assert len(first) - 1 >= 2 and len(mfma) == 0
    seqs = [rng.integers(4, cfg["vocab_size"], n).tolist() for n in lengths]
    got, ref = dec.embed(seqs), embed_ref(seqs, True)
    for i in range(len(seqs)):
        _within(got[i], ref[i], f"sequence {i} ({lengths[i]} tokens)")


def test_embed_reaches_the_tile_route(tmp_path):
    """1 600 rows at hidden 1024 / q_dim 2048 / intermediate 3072: the Q projection and gate / up have the 208 tiles the 128 x 128
    route asks for (tests/test_gpu_qwen3.py), so the packed path must advance the counter; the one sequence runs the matrix-core
    attention route."""
    import kjarni_amd
    d = str(tmp_path / "widths")
    cfg, t = F.qwen3_model(d, F.Q3_06B_WIDTHS, seed=F.MODEL_SEED, max_position_embeddings=2048)
    dec, ref = kjarni_amd.HipDecoder(d), Qwen3Ref64(t, cfg)
    rng = np.random.default_rng(4)
    seqs = [rng.integers(4, cfg["vocab_size"], 1600).tolist(), rng.integers(4, cfg["vocab_size"], 40).tolist()]
    before = dec.tile_gemm_calls()
    got = dec.embed(seqs)
    assert dec.tile_gemm_calls() - before == 3 * cfg["num_hidden_layers"]
    for i, s in enumerate(seqs):
        _within(got[i], _l2(ref.final_norm(ref.forward(s, ref.new_cache())[-1:]))[0], f"sequence {i} ({len(s)} tokens)")


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------

def test_embed_leaves_generation_state_untouched(tmp_path):
    dec, cfg, _ = _make(tmp_path, "llama")
    rng = np.random.default_rng(9)
    prompt = rng.integers(4, cfg["vocab_size"], 30).tolist()
    others = [rng.integers(4, cfg["vocab_size"], n).tolist() for n in (40, 3, 17)]
    first = dec.generate(prompt, 8)
    state = (dec.cache_len(), dec.resident(), _bits(dec.last_logits()).copy())
    kv = [tuple(a.copy() for a in dec.kv_rows(i)) for i in range(dec.layers)]
    dec.embed(others)
    assert (dec.cache_len(), dec.resident()) == state[:2] and np.array_equal(_bits(dec.last_logits()), state[2])
    for i in range(dec.layers):
        k, v = dec.kv_rows(i)
        assert np.array_equal(_bits(k), _bits(kv[i][0])) and np.array_equal(_bits(v), _bits(kv[i][1]))
    assert dec.generate(prompt, 8) == first

    # prefix reuse: the kept-row counters advance by what they advance without an embed call in between, and the ids are those
    # of the call before (the same rows are kept and the same rows recomputed)
    dec.set_prefix_reuse(True)
    dec.generate(prompt, 8)
    s0 = dec.prefix_stats()
    second = dec.generate(prompt, 8)
    s1 = dec.prefix_stats()
    dec.embed(others)
    assert dec.prefix_stats() == s1
    assert dec.generate(prompt, 8) == second
    s2 = dec.prefix_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1]) == (s1[0] - s0[0], s1[1] - s0[1]) and s1[0] - s0[0] == len(prompt) - 1


# ---- 7. validation and refusals -----------------------------------------------------------------------------------------------------

def test_embed_validates_before_any_gpu_work(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    dec, cfg, _ = _make(tmp_path, "qwen2")            # max_position_embeddings 128: the embed length limit
    V = cfg["vocab_size"]
    ids = np.arange(4, 4 + 200, dtype=np.uint32) % (V - 4) + 4
    cases = [
        (ids, [0, 5, 3, 9], ("offsets[2]", "sequence 1")),          # offsets that decrease
        (ids, [0, 5, 5, 9], ("offsets[1]", "empty", "sequence 1")),  # an empty sequence
        (ids, [0, 5, 134], ("offsets", "129", "128", "sequence 1")),  # longer than min(context, 2048)
        (ids, [-1, 3], ("offsets[0]",)),
    ]
    bad = ids.copy()
    bad[7] = V
    cases.append((bad, [0, 5, 9], ("ids[7]", str(V), "sequence 1")))
    for a, off, words in cases:
        with pytest.raises(KjarniException) as e:
            dec.embed_flat(a, off)
        assert e.value.code == E.INVALID_CONFIG and all(w in str(e.value) for w in words), str(e.value)
    assert dec.cache_len() == 0
    out = dec.embed([])
    assert out.shape == (0, cfg["hidden_size"])
    assert dec.embed_flat(ids, [0, 128]).shape == (1, cfg["hidden_size"])      # exactly the limit is fine


def test_embed_refuses_gpt2_and_quantized_checkpoints(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "gpt2")
    G2.gpt2_model(d, G2.gpt2_config(**G2.SMALL), seed=1)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.HipDecoder(d).embed([[5, 6, 7]])
    assert e.value.code == E.INVALID_CONFIG and "GPT-2" in str(e.value)
    path = str(tmp_path / "q8.gguf")
    GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.HipDecoder(path).embed([[5, 6, 7]])
    assert e.value.code == E.INVALID_CONFIG and "quantized" in str(e.value)
    d = str(tmp_path / "odd")      # hidden 48: not a multiple of 32, a geometry forward() keeps off the matrix-core route
    synth.llm_model(d, dict(synth.LLAMA_TEST, hidden_size=48, num_attention_heads=3, num_key_value_heads=1, head_dim=16, intermediate_size=96), seed=3)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.HipDecoder(d).embed([[5, 6, 7]])
    assert e.value.code == E.INVALID_CONFIG and "multiples of 32" in str(e.value)


# ---- 8. the Embedder C ABI on a decoder directory -------------------------------------------------------------------------------------

TEXTS = ["Hello world", "The quick brown fox jumps over the lazy dog.", "x", "  two  spaces and a newline\n"]


def _embedder_dir(tmp_path):
    d = str(tmp_path / "q3-embedder")
    cfg, t = F.qwen3_model(d, F.Q3_SMALL, seed=F.CHAT_MODEL_SEED, vocab_size=720, bos_token_id=700, eos_token_id=702)
    j = json.load(open(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json")))
    eot = "<|endoftext|>"
    j["post_processor"] = {"type": "TemplateProcessing", "single": [{"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": eot, "type_id": 0}}],
                           "pair": [{"Sequence": {"id": "A", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 1}}],
                           "special_tokens": {eot: {"id": eot, "ids": [700], "tokens": [eot]}}}
    with open(os.path.join(d, "tokenizer.json"), "w") as f:
        json.dump(j, f)
    return d, cfg


def test_embedder_abi_on_a_decoder_directory(tmp_path):
    import kjarni_amd
    from kjarni_amd.chat import BpeTokenizer
    d, cfg = _embedder_dir(tmp_path)
    tok = BpeTokenizer(os.path.join(d, "tokenizer.json"))
    limit = min(cfg["max_position_embeddings"], 2048)
    long_text = "word " * 400                              # more tokens than the limit: cut from the right, the appended token stays
    texts = TEXTS + [long_text]
    ids = [tok.encode_embedding(t, limit) for t in texts]
    assert all(s[-1] == 700 for s in ids) and len(ids[-1]) == limit and ids[0][:-1] == tok.encode(TEXTS[0])
    dec = kjarni_amd.HipDecoder(d)
    emb = kjarni_amd.Embedder(model_path=d)
    assert emb.dim == cfg["hidden_size"] == dec.hidden
    got = emb.encode_batch(texts)
    assert got.shape == (len(texts), dec.hidden)
    _within(got, dec.embed(ids, True), "encode_batch against HipDecoder.embed of the framed ids")
    assert np.abs(np.linalg.norm(got.astype(F64), axis=-1) - 1.0).max() < 1e-5
    raw = kjarni_amd.Embedder(model_path=d, normalize=False)
    _within(np.asarray(raw.encode(TEXTS[1]), np.float32), dec.embed([ids[1]], False)[0], "encode, normalize = 0")
    _within(raw.encode_batch([TEXTS[1]])[0], got[1], "encode_batch normalises whatever the handle says")
    _within(np.asarray(emb.encode(TEXTS[1]), np.float32), got[1], "encode, normalize = 1")
    sim = emb.similarity(TEXTS[0], TEXTS[1])
    assert abs(sim - float(got[0].astype(F64) @ got[1].astype(F64))) <= R.TOL
    assert abs(raw.similarity(TEXTS[0], TEXTS[1]) - sim) <= R.TOL        # the cosine of the un-normalised rows is the same number


def test_encoder_directory_still_loads_as_an_encoder(tmp_path):
    import kjarni_amd
    from oracle import oracle as O
    d = str(tmp_path / "minilm")
    cfg, t = synth.minilm_embedder(d, seed=3)
    synth.add_tokenizer(d)
    emb = kjarni_amd.Embedder(model_path=d)
    assert emb.dim == cfg["hidden_size"]
    tok = kjarni_amd.Tokenizer(os.path.join(d, "tokenizer.json"), 512)
    ids, mask, _ = tok.encode_batch(TEXTS[:2])
    assert np.abs(emb.encode_batch(TEXTS[:2]) - O.OracleModel(t, cfg).embed_batch(ids, mask)).max() < 1e-4      # mean pool + L2, as before


def test_embedder_refuses_a_tokenizer_it_cannot_frame(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    d, cfg = _embedder_dir(tmp_path)
    j = json.load(open(os.path.join(d, "tokenizer.json")))
    j["post_processor"] = {"type": "RobertaProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0]}
    with open(os.path.join(d, "tokenizer.json"), "w") as f:
        json.dump(j, f)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        kjarni_amd.Embedder(model_path=d)
    assert e.value.code == E.LOAD_FAILED and "unsupported post_processor 'RobertaProcessing'" in str(e.value)
