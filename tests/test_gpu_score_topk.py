"""Top-k alternatives per scored position on the GPU (kjarni_hip_decoder_score_topk, kjarni_hip_op_score_head_topk,
kjarni_generator_score_tokens).

The head kernels alone against numpy float64 on both routes (every row and slot), planted winners in the places where two
lists meet (one lane's accumulators, the two half-waves, the two waves, the slabs, the partial tile), heads whose logits are
all negative, tied logits; whole models (the fixtures of tests/test_gpu_score.py and a Qwen3 one) against the float64
references; the state score_topk() leaves and its validation; the Generator.

Bars.  tests/test_gpu_score.py's: logits carry B = 1e-4 * max(1, max |ref logits|) and lse is 1-Lipschitz in the sup norm, so
every log-probability and lse gets 2 B.  The j-th largest of a row is 1-Lipschitz in the sup norm as well, so slot j's value is
held to the j-th largest float64 log-probability with the same 2 B, whichever id the device chose among near-equal logits;
and the float64 log-probability of the id it did choose is held to the returned value.  Exact ids are compared where the
float64 logit is at least lanes_cases.GAP away from both neighbours in the sorted list (the (k+1)-th counts as one); at most
5 % of a case's slots may be left out that way.  logprob, lse and slot 0 are compared bit for bit with the plain call."""
import ctypes as C

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import qwen3_fixture as F
from tests import synth
from tests.test_gpu_lookup import _llama
from tests.test_gpu_score import (HEAD_MS, MODELS, SLAB_TILES, TIE_PAIRS, _bar, _bf16_round, _head_case, _head_launches, _log_softmax64,
                                  _model, _prompt, _targets, _w_arg)

pytestmark = pytest.mark.gpu

TOPK_SHAPES = ((64, 70), (64, 320), (96, 701), (64, 128256))
TOP_KS = (1, 2, 8)
ROUTES = tuple((True, st) for st in SLAB_TILES) + ((False, 0),)      # (fused, slab_tiles)
MASK_LIMIT = 0.05


def _sorted_ref(logits64, k):
    """The k + 1 best columns of every row, best first (equal logits: the larger column first, argmax_key's order), and their
    float64 logits."""
    x = np.asarray(logits64, np.float64)
    rows, vocab = x.shape
    kk = min(k + 1, vocab)
    rev = x[:, ::-1]                                                  # a stable sort of the reversed row puts the larger column first
    part = np.argpartition(-rev, kk - 1, axis=1)[:, :kk] if kk < vocab else np.tile(np.arange(vocab), (rows, 1))
    vals = np.take_along_axis(rev, part, axis=1)
    order = np.lexsort((part, -vals), axis=1)
    idx = vocab - 1 - np.take_along_axis(part, order, axis=1)
    return idx, np.take_along_axis(x, idx, axis=1)


def _clear_slots(sorted_vals, k):
    """[rows, k] bool: the slot's float64 logit is >= GAP away from both neighbours of the sorted list (the (k+1)-th included)."""
    gap = -np.diff(sorted_vals, axis=1)                               # gap[:, j] = s[j] - s[j + 1]
    rows, have = sorted_vals.shape
    below = np.full((rows, k), np.inf)
    below[:, :min(k, have - 1)] = gap[:, :k]
    above = np.full((rows, k), np.inf)
    above[:, 1:] = below[:, :-1]
    return (below >= LC.GAP) & (above >= LC.GAP)


def _check_topk(got, logits64, targets, k, what, ref=None, bar_factor=2.0, mask=None, mask_limit=MASK_LIMIT, lsm=None):
    """got = (logprob [rows], ids [rows, k], logprob [rows, k], lse or None) of the rows whose float64 logits are logits64.
    ref, mask, lsm: _sorted_ref, _clear_slots and _log_softmax64 of (at least) these rows where the caller has them already."""
    lp, tid, tlp, lse = got
    rows, vocab = logits64.shape
    assert lp.shape == (rows,) and tid.shape == tlp.shape == (rows, k), what
    lsm, lse64 = (lsm[0][:rows], lsm[1][:rows]) if lsm is not None else _log_softmax64(logits64)
    bar = bar_factor * _bar(logits64)
    idx, vals = ref if ref is not None else _sorted_ref(logits64, k)
    idx, vals = idx[:rows, :k], vals[:rows]
    assert np.isfinite(lp).all() and np.isfinite(tlp).all(), what
    assert (np.diff(tlp, axis=1) <= 0).all(), f"{what}: a row's values increase"
    ids = tid.astype(np.int64)
    assert (ids < vocab).all(), f"{what}: an id is not below vocab"
    srt = np.sort(ids, axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), f"{what}: an id is returned twice"
    want_lp = lsm[np.arange(rows), np.asarray(targets, np.int64)]
    errs = {
        "logprob": np.abs(lp.astype(np.float64) - want_lp).max(),
        "slot value": np.abs(tlp.astype(np.float64) - (vals[:, :k] - lse64[:, None])).max(),
        "value of the returned id": np.abs(tlp.astype(np.float64) - np.take_along_axis(lsm, ids, axis=1)).max(),
    }
    if lse is not None:
        errs["lse"] = np.abs(lse.astype(np.float64) - lse64).max()
    print(f"{what}: " + ", ".join(f"{n} err {e:.3e}" for n, e in errs.items()) + f" bar {bar:.3e}")
    for n, e in errs.items():
        assert e <= bar, f"{what}: {n}: {e:.3e} > {bar:.3e}"
    clear = _clear_slots(vals, k) if mask is None else mask[:rows]
    if mask is None:
        left_out = clear.size - int(clear.sum())
        assert left_out <= int(mask_limit * clear.size), f"{what}: {left_out} of {clear.size} slots lie within {LC.GAP} of a neighbour"
    assert (ids[clear] == idx[clear]).all(), f"{what}: ids"


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the kernels alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,vocab", TOPK_SHAPES, ids=[f"{k}x{v}" for k, v in TOPK_SHAPES])
def test_head_kernels_against_float64(k, vocab, bf16):
    from kjarni_amd import ops
    X, W, logits = _head_case(k, vocab, bf16)
    Wa = _w_arg(W, bf16)
    ref, lsm = _sorted_ref(logits, max(TOP_KS)), _log_softmax64(logits)
    masks = {}
    for top_k in TOP_KS:                                              # the mask: once per head over the 130 rows
        masks[top_k] = _clear_slots(ref[1][:, :top_k + 1], top_k)
        left_out = masks[top_k].size - int(masks[top_k].sum())
        print(f"k {k} vocab {vocab} top_k {top_k}: {left_out} of {masks[top_k].size} slots left out")
        assert left_out <= int(MASK_LIMIT * masks[top_k].size)
    for m in HEAD_MS:
        for fused, st in ROUTES:
            tg = _targets(m, vocab, st, logits[:m])
            lp0, top0, tlp0, lse0 = ops.score_head(X[:m], Wa, tg, bf16=bf16, slab_tiles=st, fused=fused)
            for top_k in TOP_KS:
                what = f"k {k} vocab {vocab} m {m} slab_tiles {st} fused {fused} top_k {top_k}"
                lp, tid, tlp, lse = ops.score_head_topk(X[:m], Wa, tg, top_k, bf16=bf16, slab_tiles=st, fused=fused)
                _check_topk((lp, tid, tlp, lse), logits[:m], tg, top_k, what, ref=(ref[0], ref[1][:, :top_k + 1]), mask=masks[top_k],
                            lsm=lsm)
                assert _same_bits(lp, lp0) and _same_bits(lse, lse0), f"{what}: logprob / lse differ from score_head's bits"
                assert np.array_equal(tid[:, 0], top0) and _same_bits(np.ascontiguousarray(tlp[:, 0]), tlp0), f"{what}: slot 0"


# ---- 2. planted winners ----------------------------------------------------------------------------------------------------------

PLANTED_C = (2.0, 1.9, 1.8, 1.7, 1.6, 1.5, 1.4, 1.3)
PLANTED_ORDER = (5, 2, 7, 0, 3, 6, 1, 4)       # column i of a placement gets PLANTED_C[PLANTED_ORDER[i]]
PLACEMENTS = (                                  # (name, vocab, the eight columns)
    ("one lane's accumulators", 320, (64, 65, 66, 67, 72, 73, 74, 75)),
    ("both half-waves and both waves", 320, tuple(range(28, 36))),
    ("one per slab", 701, tuple(64 * t + 7 * t + 1 for t in range(8))),
    ("the partial tile of 701", 701, tuple(range(693, 701))),
    ("the partial tile of 70", 70, tuple(range(62, 70))),
)


def _unit_case(k, m, seed):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(k).astype(np.float32)
    u /= np.linalg.norm(u)
    X = (5.0 * u[None, :] + rng.standard_normal((m, k), dtype=np.float32)).astype(np.float32)
    return rng, u, X


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,vocab,cols", PLACEMENTS, ids=[p[0].replace(" ", "-") for p in PLACEMENTS])
def test_planted_winners_come_back_in_order(name, vocab, cols, bf16):
    from kjarni_amd import ops
    k, m = 64, 8
    rng, u, X = _unit_case(k, m, 17)
    W = rng.standard_normal((vocab, k), dtype=np.float32) * np.float32(0.1)
    for i, col in enumerate(cols):
        W[col] = np.float32(PLANTED_C[PLANTED_ORDER[i]]) * u
    if bf16:
        W = _bf16_round(W)
    want = np.array([cols[PLANTED_ORDER.index(j)] for j in range(8)], np.int64)   # the columns in the order of c_j
    logits = X.astype(np.float64) @ W.astype(np.float64).T
    idx, vals = _sorted_ref(logits, 8)
    assert (idx[:, :8] == want[None, :]).all() and (-np.diff(vals, axis=1)).min() > 100 * 2 * _bar(logits)   # gaps far above the bar
    tg = np.full(m, cols[0], np.uint32)
    for fused, st in ROUTES:
        for top_k in (8, 3):
            what = f"{name} slab_tiles {st} fused {fused} top_k {top_k}"
            got = ops.score_head_topk(X, _w_arg(W, bf16), tg, top_k, bf16=bf16, slab_tiles=st, fused=fused)
            assert (got[1].astype(np.int64) == want[None, :top_k]).all(), f"{what}: {got[1][0]} for {want[:top_k]}"
            _check_topk(got, logits, tg, top_k, what, ref=(idx, vals[:, :top_k + 1]), mask=np.ones((m, top_k), bool))


# ---- 3. every logit negative -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("vocab", [70, 701])
def test_all_negative_logits_keep_padding_columns_out(vocab, bf16):
    """A padding column whose logit were clamped or zero-filled would beat every real one."""
    from kjarni_amd import ops
    k, m = 64, 8
    rng, u, X = _unit_case(k, m, 23)
    c = (1.0 + rng.permutation(vocab) / vocab).astype(np.float32)
    W = (-c[:, None] * u[None, :]).astype(np.float32)
    if bf16:
        W = _bf16_round(W)
    logits = X.astype(np.float64) @ W.astype(np.float64).T
    assert logits.max() < -1.0
    tg = np.arange(m, dtype=np.uint32)
    for fused, st in ROUTES:
        for top_k in (1, 8):
            what = f"all negative vocab {vocab} slab_tiles {st} fused {fused} top_k {top_k}"
            got = ops.score_head_topk(X, _w_arg(W, bf16), tg, top_k, bf16=bf16, slab_tiles=st, fused=fused)
            assert (got[1] < vocab).all() and (got[2] < 0).all(), what
            _check_topk(got, logits, tg, top_k, what, mask_limit=1.0)   # (the rows of W are close to each other by construction)


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_tied_logits_put_the_larger_index_first(bf16):
    """tests/test_gpu_score.py's pairs: identical rows of W give bit-identical logits; slots 0 and 1 are (b, a)."""
    from kjarni_amd import ops
    k, vocab, m = 64, 320, 8
    rng, u, X = _unit_case(k, m, 3)
    for a, b in TIE_PAIRS:
        W = rng.standard_normal((vocab, k), dtype=np.float32) * np.float32(0.1)
        W[a] = 2.0 * u
        W[b] = W[a]
        if bf16:
            W = _bf16_round(W)
        logits = X.astype(np.float64) @ W.astype(np.float64).T
        assert (logits[:, a] == logits[:, b]).all() and (logits[:, b] - np.delete(logits, [a, b], axis=1).max(axis=1)).min() > 1.0
        tg = np.full(m, a, np.uint32)
        for fused, st in ROUTES:
            for top_k in (2, 8):
                what = f"pair {(a, b)} slab_tiles {st} fused {fused} top_k {top_k}"
                lp, tid, tlp, lse = ops.score_head_topk(X, _w_arg(W, bf16), tg, top_k, bf16=bf16, slab_tiles=st, fused=fused)
                assert (tid[:, 0] == b).all() and (tid[:, 1] == a).all(), what
                assert np.array_equal(tlp[:, 0].view(np.uint32), tlp[:, 1].view(np.uint32)) and _same_bits(lp, np.ascontiguousarray(tlp[:, 1])), what
                assert np.abs(tlp[:, 0].astype(np.float64) - _log_softmax64(logits)[0][:, b]).max() <= 2 * _bar(logits), what


# ---- 5. whole models ---------------------------------------------------------------------------------------------------------------

MODEL_K = 5


def _topk_case(dec, ref_logits, ids, first, fused, what, bar_factor=2.0, launches=None):
    """score_topk(ids, first) against the float64 logits of the rows first - 1 .. n - 2; returns what it returned."""
    n = len(ids)
    f0, r0 = dec.score_calls()
    got = dec.score_topk(ids, first, MODEL_K)
    f1, r1 = dec.score_calls()
    want = _head_launches(n, first, fused) if launches is None else launches
    assert (f1 - f0, r1 - r0) == ((want, 0) if fused else (0, want)), f"{what}: route counters"
    _check_topk(got + (None,), ref_logits, ids[first:], MODEL_K, what, bar_factor=bar_factor)
    assert dec.cache_len() == n
    lp, top, tlp = dec.score(ids, first)                              # the plain call on the same model and route
    assert _same_bits(got[0], lp), f"{what}: logprob differs from score()'s bits"
    assert np.array_equal(got[1][:, 0], top) and _same_bits(np.ascontiguousarray(got[2][:, 0]), tlp), f"{what}: slot 0"
    return got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rows"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
def test_models_against_float64(tmp_path, name, bf16, fused):
    dec, ref = _model(tmp_path, name, bf16)
    dec.set_score_fused(fused)
    for n in (9, 40) + (() if not fused else (128 if name == "qwen2" else 130,)):
        ids = _prompt(ref, n)
        logits = ref.logits(ids, ref.new())
        for first in sorted({1, n // 2, n - 1}):
            _topk_case(dec, logits[first - 1:n - 1], ids, first, fused, f"{name} n {n} first {first} fused {fused}")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rows"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_qwen3_against_float64(tmp_path, bf16, fused):
    import kjarni_amd
    from tests.qwen3_ref64 import Qwen3Ref64
    d = str(tmp_path / "q3")
    cfg, t = F.qwen3_model(d, F.Q3_SMALL, seed=F.MODEL_SEED, store_bf16=bf16)
    dec, ref = kjarni_amd.HipDecoder(d), Qwen3Ref64(t, cfg)
    assert dec.bf16 == bf16
    dec.set_score_fused(fused)
    for n in (9, 40):
        ids = F.seeded_prompt(31, cfg["vocab_size"], n)
        logits = ref.logits(ref.forward(ids, ref.new_cache()))
        for first in (1, n // 2):
            _topk_case(dec, logits[first - 1:n - 1], ids, first, fused, f"qwen3 n {n} first {first} fused {fused}")


def test_chunk_boundary(tmp_path):
    """tests/test_gpu_score.py's case: the row at position 2 047 is scored against the id at 2 048, the next chunk's first."""
    dec, ref = _model(tmp_path, "llama", False, max_position_embeddings=2112)
    n, first = 2050, 2040
    ids = _prompt(ref, n)
    logits = ref.logits(ids, ref.new())
    _topk_case(dec, logits[first - 1:n - 1], ids, first, True, f"n {n} first {first}")


def test_rows_route_quantized_head(tmp_path):
    """tests/test_gpu_score.py's Q4_K_M fixture (Q6_K head) against the library's own per-prefix logits: both sides carry the
    device's error, at most B each in the logits, and a log-probability doubles that: 4 B."""
    from kjarni_amd import HipDecoder
    path = str(tmp_path / "m" / "model.gguf")
    cfg, _ = GG.gguf_model(path, GG.LLAMA_Q, GG.q4_k_m_types(GG.LLAMA_Q["num_hidden_layers"]), seed=7, rope_freqs=True)
    dec = HipDecoder(str(tmp_path / "m"))
    assert dec.weight_bytes_by_type().get("Q6_K", 0) > 0
    n = 12
    ids = np.random.default_rng(11).integers(4, cfg["vocab_size"], n).tolist()
    for first in (1, 6):
        rows = []
        for p in range(first, n):
            dec.reset()
            rows.append(dec.forward(ids[:p])[1].astype(np.float64))
        _topk_case(dec, np.stack(rows), ids, first, False, f"quantized first {first}", bar_factor=4.0)


def test_prefix_reuse_gives_the_same_bits(tmp_path):
    dec, ref = _model(tmp_path, "llama", False)
    A = _prompt(ref, 60)
    B = A[:33] + [t for t in np.random.default_rng(12).integers(ref.first_id, ref.vocab, 40).tolist() if t != A[33]][:20]
    fresh = dec.score_topk(B, 30, MODEL_K)
    dec.set_prefix_reuse(True)
    dec.score_topk(A, 1, MODEL_K)
    before = dec.prefix_stats()
    again = dec.score_topk(B, 30, MODEL_K)
    kept = dec.prefix_stats()[0] - before[0]
    assert kept == 29, kept                                           # first - 1 rows at most: row 29 must reach the head
    for g, w in zip(again, fresh):
        assert _same_bits(g, w)


# ---- 6. state and errors -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 40])
def test_state_after_score_topk(tmp_path, n):
    dec, ref = _model(tmp_path, "llama", False)
    ids = _prompt(ref, n)
    dec.reset()
    _, want_logits = dec.forward(ids)
    want_kv = [dec.kv_rows(i) for i in range(dec.layers)]
    want_ids = dec.generate(ids, 8)
    dec.reset()
    dec.forward([5, 6, 7], fetch=False)                 # whatever was there is gone after score_topk()
    dec.score_topk(ids, 1, 8)
    assert dec.cache_len() == n
    for (k, v), (wk, wv) in zip([dec.kv_rows(i) for i in range(dec.layers)], want_kv):
        assert np.array_equal(k, wk) and np.array_equal(v, wv)
    assert _same_bits(dec.last_logits(), want_logits)
    assert dec.generate(ids, 8) == want_ids


def test_validation(tmp_path):
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    dec, _, _ = _llama(tmp_path, synth.LLAMA_TEST, 0, max_context=48)
    tiny, _, _ = _llama(tmp_path / "tiny", dict(synth.LLAMA_TEST, vocab_size=6), 0, max_context=48)
    for d, ks in ((dec, (0, 9, -1)), (tiny, (7, 8))):
        d.reset()
        d.forward([4, 5, 4], fetch=False)
        want_kv = [d.kv_rows(i) for i in range(d.layers)]
        calls = d.score_calls()
        for top_k in ks:
            with pytest.raises(KjarniException, match="top_k") as e:
                d.score_topk([4, 5, 4, 5], 1, top_k)
            assert e.value.code == E.INVALID_CONFIG and d.cache_len() == 3, top_k
        for (k, v), (wk, wv) in zip([d.kv_rows(i) for i in range(d.layers)], want_kv):
            assert np.array_equal(k, wk) and np.array_equal(v, wv)
        assert d.score_calls() == calls
    lp, tid, tlp = tiny.score_topk([4, 5, 4, 5], 1, 6)                # top_k == vocab: every token, each once
    assert (np.sort(tid, axis=1) == np.arange(6)[None, :]).all() and (np.diff(tlp, axis=1) <= 0).all()
    for ids, first, field in (([5], 1, "n "), ([5, 6, 7], 0, "first"), ([5, 6, 2 ** 31], 2, r"ids\[2\]")):   # score()'s own errors
        with pytest.raises(KjarniException, match=field) as e:
            dec.score_topk(ids, first, 3)
        assert e.value.code == E.INVALID_CONFIG
    x, w = np.zeros((2, 32), np.float32), np.zeros((5, 32), np.float32)
    for top_k in (0, 9, 6):
        for fused in (True, False):
            with pytest.raises(KjarniException, match="top_k") as e:
                ops.score_head_topk(x, w, np.zeros(2, np.uint32), top_k, fused=fused)
            assert e.value.code == E.INVALID_CONFIG


# ---- 7. the Generator --------------------------------------------------------------------------------------------------------------

def test_generator_score_tokens(tmp_path, monkeypatch):
    from kjarni_amd import Generator, HipDecoder, _ffi
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen, dec = Generator("gpt2", model_path=d), HipDecoder(d, 0)
    L = _ffi.lib()
    pairs = [("The quick brown fox", " jumps over the lazy dog", 5), ("Hello", " world", 1), ("", "In a hole in the ground there lived", 8)]
    for context, continuation, top_k in pairs:
        whole, first = gen.encode(context + continuation), len(gen.encode(context))
        lp, tid, tlp = dec.score_topk(whole, first, top_k)
        r = _ffi.KjarniTokenScores()
        assert L.kjarni_generator_score_tokens(gen._handle, context.encode(), continuation.encode(), top_k, C.byref(r)) == 0
        assert (r.n_tokens, r.top_k) == (len(whole) - first, top_k)
        assert [r.tokens[i] for i in range(r.n_tokens)] == whole[first:]
        L.kjarni_token_scores_free(C.byref(r))
        assert not r.tokens and not r.top_logprobs and (r.n_tokens, r.top_k) == (0, 0)
        frees = []
        real_free = L.kjarni_token_scores_free
        monkeypatch.setattr(L, "kjarni_token_scores_free", lambda p: (frees.append(1), real_free(p))[1])
        tokens, logprobs, top_tokens, top_logprobs = gen.score_tokens(context, continuation, top_k)
        monkeypatch.undo()
        assert len(frees) == 1                                             # the wrapper frees what the library allocated, once
        assert tokens.tolist() == whole[first:] and top_tokens.shape == top_logprobs.shape == (len(whole) - first, top_k)
        assert _same_bits(logprobs, lp) and np.array_equal(top_tokens, tid) and _same_bits(top_logprobs, tlp)
        total = 0.0
        for v in logprobs:
            total += float(v)
        assert total == gen.score(context, continuation)[0]
    assert gen.score_tokens("Hello", " world")[2].shape[1] == 5            # the default top_k
    r = _ffi.KjarniTokenScores()
    for context, continuation, top_k, match in (("Hello", "", 5, "adds no tokens"), ("Hello", " world", 0, "top_k"), ("Hello", " world", 9, "top_k")):
        with pytest.raises(KjarniException, match=match) as e:
            _ffi.check_error(L.kjarni_generator_score_tokens(gen._handle, context.encode(), continuation.encode(), top_k, C.byref(r)))
        assert e.value.code == E.INVALID_CONFIG
        assert not r.tokens and not r.logprobs and not r.top_tokens and not r.top_logprobs and (r.n_tokens, r.top_k) == (0, 0)
