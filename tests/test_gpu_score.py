"""Scoring on the GPU (kjarni_hip_decoder_score, kjarni_hip_op_score_head, kjarni_generator_score).

The head kernels alone against numpy float64 (fused and rows route, f32 and bf16 heads, slab widths, ties, large logits);
whole models against the float64 references with every row's logits (tests/test_gpu_lookup.py's wrappers); the boundary
between two 2 048-row prompt chunks; the rows route, forced and on a quantized head; the state score() leaves and its
validation; the Generator.

Bars.  Logits carry the decoder's bar B = 1e-4 * max(1, max |ref logits|).  lse is 1-Lipschitz in the sup norm, so logprob =
x_t - lse, top_logprob and lse get 2B.  The arg-max is compared only on rows where the reference's two best logits are at
least lanes_cases.GAP apart; at most 2 % of a case's rows may be left out that way, none in a case of fewer than 50 rows."""
import functools

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import synth
from tests.test_gpu_lookup import _Gpt264, _Llama64, _llama

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _bar(ref_logits):
    return TOL * max(1.0, float(np.abs(ref_logits).max()))


def _log_softmax64(logits):
    """Per row: (log-softmax [rows, vocab], lse [rows]) in float64, log_softmax_1d's formula."""
    x = np.asarray(logits, np.float64)
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    return x - lse[:, None], lse


def _last_max_rows(x):
    return (x.shape[1] - 1 - np.argmax(x[:, ::-1], axis=1)).astype(np.int64)


def _gaps(x):
    top = np.partition(x, -2, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0]


def _check_rows(got, logits64, targets, what, bar_factor=2.0, lse=None):
    """got = (logprob, top, top_logprob) of the rows whose float64 logits are logits64 [rows, vocab]."""
    lp, top, tlp = got
    rows = logits64.shape[0]
    assert lp.shape == top.shape == tlp.shape == (rows,), what
    lsm, lse64 = _log_softmax64(logits64)
    bar = bar_factor * _bar(logits64)
    want_lp = lsm[np.arange(rows), np.asarray(targets, np.int64)]
    want_top = _last_max_rows(logits64)
    want_tlp = lsm[np.arange(rows), want_top]
    for name, g, w in (("logprob", lp, want_lp), ("top_logprob", tlp, want_tlp)) + ((("lse", lse, lse64),) if lse is not None else ()):
        err = float(np.abs(np.asarray(g, np.float64) - w).max())
        print(f"{what}: {name} err {err:.3e} bar {bar:.3e}")
        assert np.isfinite(g).all() and err <= bar, f"{what}: {name}: {err:.3e} > {bar:.3e}"
    clear = _gaps(logits64) >= LC.GAP
    left_out = int(rows - clear.sum())
    assert left_out <= (0 if rows < 50 else int(0.02 * rows)), f"{what}: {left_out} of {rows} rows have their two best logits within {LC.GAP}"
    assert (top[clear].astype(np.int64) == want_top[clear]).all(), f"{what}: arg-max"


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------

HEAD_MS = (1, 8, 63, 64, 65, 130)
HEAD_SHAPES = ((64, 320), (96, 701), (768, 50257), (64, 128256))
SLAB_TILES = (0, 1, 3)


def _bf16_round(a):
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def _w_arg(W, bf16):
    return (W.view(np.uint32) >> 16).astype(np.uint16) if bf16 else W


@functools.lru_cache(maxsize=2)
def _head_case(k, vocab, bf16):
    """hidden [130, k], W [vocab, k] (bf16-representable when bf16) and the float64 logits of all 130 rows, computed once."""
    rng = np.random.default_rng(1000 * k + vocab % 997)
    X = rng.standard_normal((max(HEAD_MS), k), dtype=np.float32)
    W = (rng.standard_normal((vocab, k), dtype=np.float32) * np.float32(0.1))
    if bf16:
        W = _bf16_round(W)
    logits = X.astype(np.float64) @ W.astype(np.float64).T
    for a in (X, W, logits):
        a.setflags(write=False)
    return X, W, logits


def _auto_slab_tiles(m, vocab):
    n_tiles, m_tiles = -(-vocab // 64), -(-m // 64)
    slabs = max(1, min(n_tiles, -(-1024 // m_tiles)))
    return -(-n_tiles // slabs)


def _targets(m, vocab, slab_tiles, logits64):
    """0, vocab - 1, columns 63 and 64, a slab's last and first column, the row's arg-max -- in turn, starting at another one
    for every m."""
    st = slab_tiles or _auto_slab_tiles(m, vocab)
    edge = min(st * 64, vocab - 1)
    special = [0, vocab - 1, 63, 64, edge - 1, edge, None]
    am = _last_max_rows(logits64)
    return np.array([am[r] if special[(r + m) % 7] is None else special[(r + m) % 7] for r in range(m)], np.uint32)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,vocab", HEAD_SHAPES, ids=[f"{k}x{v}" for k, v in HEAD_SHAPES])
def test_head_kernels_against_float64(k, vocab, bf16):
    from kjarni_amd import ops
    X, W, logits = _head_case(k, vocab, bf16)
    Wa = _w_arg(W, bf16)
    for m in HEAD_MS:
        for fused, slabs in ((True, SLAB_TILES), (False, (0,))):
            for st in slabs:
                tg = _targets(m, vocab, st, logits[:m])
                lp, top, tlp, lse = ops.score_head(X[:m], Wa, tg, bf16=bf16, slab_tiles=st, fused=fused)
                _check_rows((lp, top, tlp), logits[:m], tg, f"k {k} vocab {vocab} m {m} slab_tiles {st} fused {fused}", lse=lse)


TIE_PAIRS = ((5, 9), (5, 37), (5, 40), (5, 70), (70, 200), (5, 319), (63, 64))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_head_ties_go_to_the_larger_index(bf16):
    """The winning row of W duplicated inside a tile (same and other wave), in another tile of the slab, in another slab:
    identical rows give bit-identical logits (the MFMA chain is k-ordered), and the larger index wins on both routes."""
    from kjarni_amd import ops
    k, vocab, m = 64, 320, 8
    rng = np.random.default_rng(3)
    u = rng.standard_normal(k).astype(np.float32)
    u /= np.linalg.norm(u)
    X = (5.0 * u[None, :] + rng.standard_normal((m, k), dtype=np.float32)).astype(np.float32)
    for a, b in TIE_PAIRS:
        W = rng.standard_normal((vocab, k), dtype=np.float32) * np.float32(0.1)
        W[a] = 2.0 * u
        W[b] = W[a]
        if bf16:
            W = _bf16_round(W)
        logits = X.astype(np.float64) @ W.astype(np.float64).T
        lsm, _ = _log_softmax64(logits)
        assert (_last_max_rows(logits) == b).all() and (logits[:, a] == logits[:, b]).all()
        others = np.delete(logits, [a, b], axis=1).max(axis=1)
        assert (logits[:, b] - others).min() > 1.0                      # nothing else comes near the pair
        tg = np.full(m, a, np.uint32)
        for fused, slabs in ((True, SLAB_TILES), (False, (0,))):
            for st in slabs:
                lp, top, tlp, lse = ops.score_head(X, _w_arg(W, bf16), tg, bf16=bf16, slab_tiles=st, fused=fused)
                what = f"pair {(a, b)} slab_tiles {st} fused {fused}"
                assert (top == b).all(), what
                assert (lp == tlp).all(), what                                 # the two logits are the same bits
                assert np.abs(tlp - lsm[:, b]).max() <= 2 * _bar(logits), what


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,vocab", HEAD_SHAPES[:2], ids=[f"{k}x{v}" for k, v in HEAD_SHAPES[:2]])
def test_head_large_logits_stay_finite(k, vocab, bf16):
    """Rows scaled until max |logit| exceeds 100, where exp() without the maximum subtracted overflows."""
    from kjarni_amd import ops
    X, W, logits = _head_case(k, vocab, bf16)
    m = 65
    scale = np.float32(150.0 / np.abs(logits[:m]).max())
    Xs = (X[:m] * scale).astype(np.float32)
    big = Xs.astype(np.float64) @ W.astype(np.float64).T
    assert np.abs(big).max() > 100.0
    tg = _targets(m, vocab, 1, big)
    for fused, slabs in ((True, SLAB_TILES), (False, (0,))):
        for st in slabs:
            lp, top, tlp, lse = ops.score_head(Xs, _w_arg(W, bf16), tg, bf16=bf16, slab_tiles=st, fused=fused)
            _check_rows((lp, top, tlp), big, tg, f"large logits k {k} vocab {vocab} slab_tiles {st} fused {fused}", lse=lse)


# ---- 2. whole models against float64 ---------------------------------------------------------------------------------------------

SHORT_LENS, PROMPT_LENS = (2, 8, 9, 23), (24, 40, 65, 130)
MODELS = ("llama", "qwen2", "gpt2")


def _model(tmp_path, name, bf16, **over):
    """(decoder, float64 reference with every row's logits), weights seed 0."""
    if name == "gpt2":
        from kjarni_amd import HipDecoder
        cfg = G.gpt2_config(**dict(G.SMALL, n_ctx=160))
        d = str(tmp_path / f"gpt2-{int(bf16)}")
        _, t = G.gpt2_model(d, cfg, seed=0, store_bf16=bf16)
        dec, ref = HipDecoder(d, 0), _Gpt264(t, cfg)
    else:
        base = dict(synth.LLAMA_TEST if name == "llama" else synth.QWEN_TEST, **over)
        dec, t, cfg = _llama(tmp_path, base, 0, store_bf16=bf16)
        ref = _Llama64(t, cfg)
    assert dec.bf16 == bf16
    return dec, ref


def _prompt(ref, n):
    return np.random.default_rng(11).integers(ref.first_id, ref.vocab, n).tolist()


def _head_launches(n, first, fused):
    """Head launches of score(ids[:n], first): the rows first - 1 .. n - 2, block by block (8-row passes below 24 tokens, else
    one 2 048-row chunk at a time; the rows route takes 8 rows per launch)."""
    lo, hi = first - 1, n - 2
    step = 8 if n < 24 else 2048
    count = 0
    for i in range(0, n, step):
        a, b = max(i, lo), min(i + step - 1, n - 1, hi)
        if a <= b:
            count += 1 if fused or n < 24 else -(-(b - a + 1) // 8)
    return count


def _score_case(dec, ref, n, first, fused, logits_cache):
    ids = _prompt(ref, n)
    if n not in logits_cache:
        logits_cache[n] = ref.logits(ids, ref.new())
    f0, r0 = dec.score_calls()
    got = dec.score(ids, first)
    f1, r1 = dec.score_calls()
    want = _head_launches(n, first, fused)
    assert (f1 - f0, r1 - r0) == ((want, 0) if fused else (0, want)), f"n {n} first {first}: route counters"
    _check_rows(got, logits_cache[n][first - 1:n - 1], ids[first:], f"n {n} first {first} fused {fused}")
    assert dec.cache_len() == n


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_models_fused_route_against_float64(tmp_path, name, bf16):
    dec, ref = _model(tmp_path, name, bf16)
    cache = {}
    for n in SHORT_LENS + PROMPT_LENS:
        n = 128 if (name == "qwen2" and n == 130) else n
        for first in sorted({1, n // 2, n - 1}):
            _score_case(dec, ref, n, first, True, cache)


# ---- 3. the boundary between two prompt chunks -------------------------------------------------------------------------------

def test_chunk_boundary(tmp_path):
    dec, ref = _model(tmp_path, "llama", False, max_position_embeddings=2112)
    cache = {}
    for first in (1, 2040):   # the row at position 2 047 is scored against the id at 2 048, the first of the next chunk
        _score_case(dec, ref, 2050, first, True, cache)


# ---- 4. the rows route ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_rows_route_forced(tmp_path, name, bf16):
    dec, ref = _model(tmp_path, name, bf16)
    dec.set_score_fused(False)
    cache = {}
    for n in (9, 40):
        for first in sorted({1, n // 2, n - 1}):
            _score_case(dec, ref, n, first, False, cache)


def test_rows_route_quantized_head(tmp_path):
    """Q4_K_M mix (Q6_K table = the tied head): against the library's own per-prefix logits, reset + forward(ids[:p]), with
    log-softmax in float64.  Both sides carry the device's error, at most B each in the logits, and the log-probability
    doubles that: 4B."""
    from kjarni_amd import HipDecoder
    path = str(tmp_path / "m" / "model.gguf")
    cfg, _ = GG.gguf_model(path, GG.LLAMA_Q, GG.q4_k_m_types(GG.LLAMA_Q["num_hidden_layers"]), seed=7, rope_freqs=True)
    dec = HipDecoder(str(tmp_path / "m"))
    assert dec.weight_bytes_by_type().get("Q6_K", 0) > 0
    n = 12
    ids = np.random.default_rng(11).integers(4, cfg["vocab_size"], n).tolist()
    for first in (1, 6, 11):
        rows = []
        for p in range(first, n):
            dec.reset()
            rows.append(dec.forward(ids[:p])[1].astype(np.float64))
        f0, r0 = dec.score_calls()
        got = dec.score(ids, first)
        f1, r1 = dec.score_calls()
        assert (f1 - f0, r1 - r0) == (0, _head_launches(n, first, False))
        _check_rows(got, np.stack(rows), ids[first:], f"quantized first {first}", bar_factor=4.0)


# ---- 5. state and validation ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 40])
def test_state_after_score(tmp_path, n):
    dec, ref = _model(tmp_path, "llama", False)
    ids = _prompt(ref, n)
    dec.reset()
    dec.forward(ids, fetch=False)
    want_kv = [dec.kv_rows(i) for i in range(dec.layers)]
    want_ids = dec.generate(ids, 8)
    dec.reset()
    dec.forward([5, 6, 7], fetch=False)                 # whatever was there is gone after score()
    dec.score(ids)
    assert dec.cache_len() == n
    for (k, v), (wk, wv) in zip([dec.kv_rows(i) for i in range(dec.layers)], want_kv):
        assert np.array_equal(k, wk) and np.array_equal(v, wv)
    assert dec.generate(ids, 8) == want_ids


def test_validation(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException   # (its text is kjarni_last_error_message)
    dec, _, _ = _llama(tmp_path, synth.LLAMA_TEST, 0, max_context=48)
    assert dec.context == 48
    dec.reset()
    dec.forward([5, 6, 7], fetch=False)
    f0 = dec.score_calls()
    for ids, first, field in (([5], 1, "n "), ([5, 6, 7], 0, "first"), ([5, 6, 7], 3, "first"), ([5, 6, 7], -1, "first"),
                              (list(range(4, 4 + 49)), 1, "context"), ([5, 320, 7], 1, r"ids\[1\]"), ([5, 6, 2 ** 31], 2, r"ids\[2\]")):
        with pytest.raises(KjarniException, match=field) as e:
            dec.score(ids, first)
        assert e.value.code == E.INVALID_CONFIG and dec.cache_len() == 3, (ids[:4], first)
    assert dec.score_calls() == f0


# ---- 6. the Generator ----------------------------------------------------------------------------------------------------------

def test_generator_score(tmp_path):
    from kjarni_amd import Generator, HipDecoder
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen, dec = Generator("gpt2", model_path=d), HipDecoder(d, 0)
    pairs = [("The quick brown fox", " jumps over the lazy dog"), ("Hello", " world"), ("Once upon a time there was a small", " house"),
             ("", "In a hole in the ground there lived")]
    for context, continuation in pairs:
        whole, first = gen.encode(context + continuation), len(gen.encode(context))
        assert first >= 1                                                  # (an empty context is the BOS token alone)
        lp, top, _ = dec.score(whole, first)
        s, cnt, greedy = gen.score(context, continuation)
        want = 0.0
        for v in lp:
            want += float(v)
        assert s == want and cnt == len(whole) - first and greedy == bool((top == np.asarray(whole[first:], np.uint32)).all())
    assert len(gen.encode("")) == 1 and gen.score("", "Hello")[1] == len(gen.encode("Hello")) - 1   # BOS alone is the context
    with pytest.raises(KjarniException, match="adds no tokens") as e:
        gen.score("Hello", "")
    assert e.value.code == E.INVALID_CONFIG
    long = " the" * 200
    assert len(gen.encode("Hello" + long)) > gen.context_size
    with pytest.raises(KjarniException, match="context of") as e:
        gen.score("Hello", long)
    assert e.value.code == E.INVALID_CONFIG
