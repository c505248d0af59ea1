"""The scoring head on the bf16 matrix cores (fused = 2 of the op hooks, set_score_fused(2)) against float64 with test_gpu_score's inputs
and bar: one / an odd number of k tiles, vocabularies ending in either half of a 128-column tile and on its 64-column boundary, rows around
the 64-row tile, slabs of an odd number of 64-column units; top-k; logits only the third bf16 plane carries; whole models."""
import numpy as np
import pytest

from tests import lanes_cases as LC
from tests.test_gpu_score import (SLAB_TILES, _bar, _check_rows, _gaps, _head_case, _model, _prompt, _targets, _w_arg)
from tests.test_gpu_score_topk import _check_topk, _same_bits
from tests.test_score_bf16_host import third_plane_case

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 130)
SHAPES = ((32, 320), (64, 200), (96, 701), (768, 50257), (64, 128256))   # (k, vocab); 200 = 128 + 64 + 8: ends in the second half-tile


def _head(X, W, tg, st=0, top_k=0):
    from kjarni_amd import ops
    fn, args = (ops.score_head_topk, (top_k,)) if top_k else (ops.score_head, ())
    return fn(X, _w_arg(W, True), tg, *args, bf16=True, slab_tiles=st, fused=2)


@pytest.mark.parametrize("k,vocab", SHAPES, ids=[f"{k}x{v}" for k, v in SHAPES])
def test_head_against_float64(k, vocab):
    X, W, logits = _head_case(k, vocab, True)
    for m in MS if vocab < 100000 else (64,):                           # (the largest vocabulary once, at the automatic slab width)
        for st in SLAB_TILES if vocab < 100000 else (0,):
            tg = _targets(m, vocab, st, logits[:m])
            lp, top, tlp, lse = _head(X[:m], W, tg, st)
            _check_rows((lp, top, tlp), logits[:m], tg, f"bf16 head k {k} vocab {vocab} m {m} slab_tiles {st}", lse=lse)
            same = zip((lp, top, tlp, lse), _head(X[:m], W, tg, st))                         # the same call twice: the same bits
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in same)


@pytest.mark.parametrize("k,vocab", SHAPES[1:3], ids=[f"{k}x{v}" for k, v in SHAPES[1:3]])
@pytest.mark.parametrize("top_k", [1, 8])
def test_head_topk(k, vocab, top_k):
    X, W, logits = _head_case(k, vocab, True)
    for m in (65, 130):
        for st in SLAB_TILES:
            tg = _targets(m, vocab, st, logits[:m])
            lp0, top0, tlp0, lse0 = _head(X[:m], W, tg, st)
            lp, tid, tlp, lse = _head(X[:m], W, tg, st, top_k)
            what = f"bf16 head k {k} vocab {vocab} m {m} slab_tiles {st} top_k {top_k}"
            _check_topk((lp, tid, tlp, lse), logits[:m], tg, top_k, what)
            assert _same_bits(lp, lp0) and _same_bits(lse, lse0), f"{what}: logprob / lse differ from the plain call's bits"
            assert np.array_equal(tid[:, 0], top0) and _same_bits(np.ascontiguousarray(tlp[:, 0]), tlp0), f"{what}: slot 0"


def test_third_plane_reaches_the_logits():
    """With plane 3 dropped every logit of third_plane_case is 0 (tests/test_score_bf16_host.py) and every log-probability -log(vocab)."""
    X, W, logits = third_plane_case()
    tg, bar = np.argmax(logits, axis=1).astype(np.uint32), 2 * _bar(logits)
    want = logits.max(axis=1) - np.log(np.exp(logits).sum(axis=1))
    assert np.abs(-np.log(logits.shape[1]) - want).min() > 100 * bar                                # what a kernel without plane 3 would miss by
    for st in (0, 1):
        lp, _, tlp, _ = _head(X, W, tg, st)
        err = float(np.abs(lp.astype(np.float64) - want).max())
        print(f"third plane slab_tiles {st}: logprob err {err:.3e} bar {bar:.3e}")
        assert err <= bar and _same_bits(lp, tlp)


def test_nan_rows_of_the_same_row_tile_stay_out():
    """The hook has no leading dimensions: what a row must not read is its neighbours in the row tile (lane == row)."""
    X, W, logits = _head_case(96, 701, True)
    tg = _targets(64, 701, 0, logits[:64])
    Xn = X[:64].copy()
    Xn[63] = np.nan
    clean, dirty = _head(X[:63], W, tg[:63]), _head(Xn, W, tg)
    assert all(np.array_equal(a.view(np.uint32), b[:63].view(np.uint32)) for a, b in zip(clean, dirty))


def _kv(dec):
    return [np.concatenate([a.view(np.uint32).ravel() for a in dec.kv_rows(i)]) for i in range(dec.layers)]

@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", ["llama", "gpt2"])
def test_models_under_setting_2(tmp_path, name, bf16):
    dec, ref = _model(tmp_path, name, bf16)
    for n in (9, 40, 130):
        ids = _prompt(ref, n)
        logits = ref.logits(ids, ref.new())
        dec.set_score_fused(1)
        want = dec.score(ids)
        kv1, calls, mine = _kv(dec), dec.score_calls(), dec.score_bf16_calls()
        dec.set_score_fused(2)
        for first in (n // 2, 1):
            got = dec.score(ids, first)
            _check_rows(got, logits[first - 1:n - 1], ids[first:], f"{name} bf16 {bf16} n {n} first {first} setting 2")
        assert all(np.array_equal(a, b) for a, b in zip(kv1, _kv(dec))) and dec.cache_len() == n
        if bf16:                                                       # the route's own counter moves, the others do not
            assert dec.score_bf16_calls() > mine and dec.score_calls() == calls
        else:                                                          # an f32 head does exactly what setting 1 does
            assert dec.score_bf16_calls() == 0 and dec.score_calls()[0] > calls[0]
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want, got))


def test_score_batch_follows_the_setting(tmp_path):
    # both sides are within 2B of float64, so of each other within 4B; the arg-max is compared where float64's is clear
    dec, ref = _model(tmp_path, "llama", True)
    dec.set_score_fused(2)
    seqs, firsts = [_prompt(ref, n) for n in (9, 40, 70)], [1, 20, 3]
    lp, tid, tlp = dec.score_batch(seqs, firsts)
    assert dec.score_bf16_calls() > 0 and dec.score_calls() == (0, 0)
    at = 0
    for ids, first in zip(seqs, firsts):
        logits = ref.logits(ids, ref.new())[first - 1:len(ids) - 1]
        rows, at = slice(at, at + len(ids) - first), at + len(ids) - first
        alone, clear = dec.score(ids, first), _gaps(logits) >= LC.GAP
        assert np.abs(lp[rows] - alone[0]).max() <= 4 * _bar(logits) and np.array_equal(tid[rows, 0][clear], alone[1][clear])
