"""Generation log-probabilities, host side (no GPU): the new symbols, their arities and what they do with NULL; every refusal
that needs no device, with the outputs found untouched; the float64 rule (tests/gen_logprobs_ref64.py) on rows worked out by
hand; the slab rule against a table worked out by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from tests import gen_logprobs_ref64 as R

SYMBOLS = {"kjarni_hip_token_logprob_slabs": 2, "kjarni_hip_op_token_logprobs_bench": 8, "kjarni_hip_op_token_logprobs": 13, "kjarni_hip_decoder_generate_logprobs": 17,
           "kjarni_hip_decoder_generate_wide_logprobs": 18, "kjarni_hip_generator_set_logprobs": 2, "kjarni_hip_chat_set_logprobs": 2,
           "kjarni_hip_generator_last_logprobs": 3, "kjarni_hip_chat_last_logprobs": 2}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kjarni_hip.h")
u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731


# ---- 1. symbols and NULL behaviour -----------------------------------------------------------------------------------------------

def test_symbols_and_arities():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    for name in ("generate_logprobs", "generate_wide_logprobs"):
        assert callable(getattr(kjarni_amd.HipDecoder, name)), name
    assert callable(ops.token_logprobs) and callable(ops.token_logprob_slabs)
    for cls in (kjarni_amd.Generator, kjarni_amd.Chat):
        assert callable(cls.set_logprobs) and callable(cls.last_logprobs)


def test_the_header_declares_what_ffi_mirrors():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, argc in SYMBOLS.items():
        m = re.search(r"\b(\w[\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in kjarni_hip.h"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == argc, name
        assert (_ffi.SIGNATURES[name][0] is C.c_int32) == ("KjarniErrorCode" in m.group(1) or "int32_t" in m.group(1)), name
    assert re.search(r"#define\s+KJARNI_SCORE_TOPK_MAX\s+8", text)
    # the sampling options keep their layout: top_k of the records travels as an argument of its own
    assert "logprob" not in re.search(r"typedef struct KjarniHipSamplingOptions \{(.*?)\}", text, re.S).group(1)


def _options(max_new=4):
    o = _ffi.KjarniHipSamplingOptions()
    o.max_new_tokens, o.repetition_penalty = max_new, 1.0
    return o


def test_generate_logprobs_null_and_refusals_without_a_device():
    L = kjarni_amd.lib()
    gen = L.kjarni_hip_decoder_generate_logprobs
    o = _options()
    p, out, cnt = np.array([5, 6, 7], np.uint32), np.full(4, 77, np.uint32), C.c_size_t(7)
    lp, ids, tlp = np.full(4, 3.5, np.float32), np.full((4, 2), 77, np.uint32), np.full((4, 2), 3.5, np.float32)
    cb = _ffi.KjarniTokenCallbackFn()
    cres, gres = _ffi.KjarniHipConstraintResult(9, 9, 9, 9, 9), _ffi.KjarniHipGrammarResult(9, 9, 9, 9, 9, 9, 9)

    def call(d=None, con=None, gram=None, opt=o, k=2, n=cnt):
        return gen(d, con, gram, u32(p), 3, C.byref(opt) if opt is not None else None, k, cb, None, u32(out), 4,
                   C.byref(n) if n is not None else None, f32(lp), u32(ids), f32(tlp), C.byref(cres), C.byref(gres))

    def untouched():
        return (out == 77).all() and (lp == 3.5).all() and (ids == 77).all() and (tlp == 3.5).all()

    assert call() == E.NULL_POINTER                      # no decoder
    assert cnt.value == 0 and untouched()
    assert (cres.final_state, cres.accepted, cres.complete, cres.violated) == (0, 0, 0, 0)
    assert (gres.final_state, gres.final_depth, gres.accepted, gres.complete, gres.violated) == (0, 0, 0, 0, 0)
    assert call(opt=None) == E.NULL_POINTER
    assert call(n=None) == E.NULL_POINTER
    for k in (-1, 9, 1 << 20):                            # judged ahead of the handle
        cnt.value = 7
        assert call(k=k) == E.INVALID_CONFIG and "top_k" in _ffi.last_error(), k
        assert cnt.value == 0 and untouched()
    fake_c, fake_g = C.c_void_p(8), C.c_void_p(16)       # never dereferenced: the pair is refused as a pair
    assert call(con=fake_c, gram=fake_g) == E.INVALID_CONFIG and "not both" in _ffi.last_error()
    assert untouched()
    o2 = _options()
    u = np.zeros(2, np.float32)
    o2.uniforms, o2.n_uniforms = f32(u), 2
    assert call(opt=o2) == E.INVALID_CONFIG and "n_uniforms" in _ffi.last_error()
    assert untouched()


def test_wide_and_handle_entries_null_behaviour():
    L = kjarni_amd.lib()
    cb = _ffi.KjarniBatchTokenCallbackFn()
    wide = L.kjarni_hip_decoder_generate_wide_logprobs
    assert wide(None, None, None, 2, None, 1.0, 0, 0, 0, cb, None, None, 4, None, 2, None, None, None) == E.NULL_POINTER
    for k in (-1, 9):     # judged ahead of the handle
        assert wide(None, None, None, 2, None, 1.0, 0, 0, 0, cb, None, None, 4, None, k, None, None, None) == E.INVALID_CONFIG
        assert "top_k" in _ffi.last_error()
    assert L.kjarni_hip_generator_set_logprobs(None, 2) == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_logprobs(None, 2) == E.NULL_POINTER
    r = _ffi.KjarniTokenScores()
    assert L.kjarni_hip_generator_last_logprobs(None, 0, C.byref(r)) == E.NULL_POINTER
    assert L.kjarni_hip_chat_last_logprobs(None, C.byref(r)) == E.NULL_POINTER
    assert L.kjarni_hip_chat_last_logprobs(None, None) == E.NULL_POINTER


# ---- 2. the op's refusals: before a device is asked for, outputs untouched -------------------------------------------------------

def _op_call(logits, calls, rows, ld, vocab, tokens, top_k, outs):
    lp, ids, tlp, lse = outs
    slabs = C.c_int32(-5)
    rc = kjarni_amd.lib().kjarni_hip_op_token_logprobs(0, f32(logits) if logits is not None else None, calls, rows, ld, vocab,
                                                       i32(tokens) if tokens is not None else None, top_k,
                                                       f32(lp) if lp is not None else None, u32(ids), f32(tlp), f32(lse), C.byref(slabs))
    return rc, slabs.value


def test_op_refusals_without_a_device():
    lg = np.zeros((1, 2, 12), np.float32)
    tk = np.array([[1, -1]], np.int32)

    def outs():
        return [np.full((1, 2), 3.5, np.float32), np.full((1, 2, 2), 77, np.uint32), np.full((1, 2, 2), 3.5, np.float32),
                np.full((1, 2), 3.5, np.float32)]

    def untouched(o):
        return (o[0] == 3.5).all() and (o[1] == 77).all() and (o[2] == 3.5).all() and (o[3] == 3.5).all()

    o = outs()
    assert _op_call(None, 1, 2, 12, 10, tk, 2, o)[0] == E.NULL_POINTER
    assert _op_call(lg, 1, 2, 12, 10, None, 2, o)[0] == E.NULL_POINTER
    assert _op_call(lg, 1, 2, 12, 10, tk, 2, [None] + o[1:])[0] == E.NULL_POINTER
    bad = [dict(calls=-1), dict(vocab=0), dict(ld=9), dict(rows=0), dict(rows=65), dict(top_k=-1), dict(top_k=9),
           dict(top_k=4, vocab=3, ld=12, tokens=np.array([[1, -1]], np.int32)), dict(tokens=np.array([[10, 0]], np.int32)),
           dict(tokens=np.array([[0, -2]], np.int32))]
    for kw in bad:
        a = dict(calls=1, rows=2, ld=12, vocab=10, tokens=tk, top_k=2)
        a.update(kw)
        rc, slabs = _op_call(lg, a["calls"], a["rows"], a["ld"], a["vocab"], a["tokens"], a["top_k"], o)
        assert rc == E.INVALID_CONFIG, kw
        assert slabs == -5 and untouched(o), kw
    _op_call(lg, 1, 2, 12, 10, tk, 9, o)
    assert "top_k" in _ffi.last_error()
    a, b = C.c_float(-1), C.c_float(-1)
    bench = kjarni_amd.lib().kjarni_hip_op_token_logprobs_bench
    assert bench(0, None, 1, 12, 2, 5, C.byref(a), C.byref(b)) == E.NULL_POINTER
    for rows, vocab, k, iters in ((0, 12, 2, 5), (65, 12, 2, 5), (2, 0, 2, 5), (2, 12, 0, 5), (2, 12, 9, 5), (2, 4, 8, 5), (2, 12, 2, 0)):
        assert bench(0, f32(lg), rows, vocab, k, iters, C.byref(a), C.byref(b)) == E.INVALID_CONFIG, (rows, vocab, k, iters)
    assert a.value == -1 and b.value == -1
    _op_call(lg, 1, 2, 12, 10, np.array([[10, 0]], np.int32), 2, o)
    assert "tokens[0]" in _ffi.last_error()


# ---- 3. the float64 rule on rows worked out by hand ----------------------------------------------------------------------------------

def test_reference_all_equal_row():
    for x, V in ((0.0, 8), (3.25, 257), (-60.0, 1000)):
        row = np.full(V, x)
        assert R.lse64(row) == pytest.approx(x + math.log(V), abs=1e-12)
        rec = R.record(row, 5, 8)
        assert rec["logprob"] == pytest.approx(-math.log(V), abs=1e-12)
        assert rec["topk_ids"].tolist() == list(range(V - 1, V - 9, -1))       # equal values: the larger id first
        assert np.allclose(rec["topk_logprob"], -math.log(V), atol=1e-12)


def test_reference_one_dominant_logit():
    V = 100
    row = np.zeros(V)
    row[17] = 50.0
    want_lse = 50.0 + math.log1p((V - 1) * math.exp(-50.0))
    rec = R.record(row, 17, 2)
    assert rec["lse"] == pytest.approx(want_lse, abs=1e-12)
    assert rec["logprob"] == pytest.approx(50.0 - want_lse, abs=1e-12) and rec["logprob"] > -1e-19 - 1e-12
    assert rec["topk_ids"].tolist() == [17, 99]
    assert R.record(row, 3, 0)["logprob"] == pytest.approx(-want_lse, abs=1e-12)
    # +88: exp(88) overflows float32's neighbourhood of use without the max subtracted; float64 holds it, the rule does not care
    row[17] = 88.0
    assert R.record(row, 17, 1)["logprob"] == pytest.approx(-math.log1p(99 * math.exp(-88.0)), abs=1e-12)


def test_reference_ties_and_the_two_zeros():
    row = np.array([0.0, -0.0, 1.0, 1.0, -1.0, np.float64("-inf")])
    assert R.topk_ids(row, 6).tolist() == [3, 2, 1, 0, 4, 5]
    lse = math.log(2 * math.e + 2 + math.exp(-1))
    rec = R.record(row, 1, 4)
    assert rec["lse"] == pytest.approx(lse, abs=1e-12)
    assert rec["logprob"] == pytest.approx(-lse, abs=1e-12)
    assert np.allclose(rec["topk_logprob"], [1 - lse, 1 - lse, -lse, -lse], atol=1e-12)
    assert R.record(row, 5, 0)["logprob"] == -np.inf
    assert R.topk_ids(np.array([np.nan, -5.0, np.nan, 2.0]), 2).tolist() == [3, 1]      # NaN lowest
    # clear_slots: slot j is left out when a neighbour in the sorted order is closer than the gap
    assert R.clear_slots(np.array([5.0, 3.0, 3.0, 1.0, 0.0]), 3, 1e-3).tolist() == [True, False, False]
    assert R.clear_slots(np.array([5.0, 3.0, 2.0, 1.0]), 4, 1e-3).tolist() == [True, True, True, True]


def test_reference_run_record():
    rows = [np.array([0.0, 1.0, 2.0]), np.array([5.0, 5.0, 0.0]), np.array([9.0, 0.0, 0.0])]
    got = R.run_record(rows, [2, 0], 2)
    assert got["logprob"].shape == (2,) and got["topk_ids"].tolist() == [[2, 1], [1, 0]]
    assert got["logprob"][0] == pytest.approx(2 - math.log(1 + math.e + math.e ** 2), abs=1e-12)
    assert got["logprob"][1] == pytest.approx(5 - math.log(2 * math.exp(5) + 1), abs=1e-12)
    assert R.run_record(rows, [], 2)["topk_ids"].shape == (0, 2)


# ---- 4. the slab rule ------------------------------------------------------------------------------------------------------------------

# (rows, vocab): slabs.  want = min(64, ceil(vocab / 1024), max(1, ceil(512 / rows))); length = ceil(vocab / want) rounded up to a
# multiple of 4; slabs = ceil(vocab / length).
#   (1, 1025): want 2, 513 -> 516, 2.       (1, 128256): want 64, 2004, 64.      (1, 151936): want 64, 2374 -> 2376, 64.
#   (9, 128256): want 57, 2251 -> 2252, 57. (64, 128256): want 8, 16032, 8.      (64, 151936): want 8, 18992, 8.
#   (64, 5000): want 5, 1000, 5.            (3, 4097): want 5, 820, 5.           (1, 4096): want 4, 1024, 4.
#   (1, 65536 + 1): want 64, 1025 -> 1028, ceil(65537 / 1028) = 64.              (2, 300000): want 64, 4688, 64.
SLAB_TABLE = {(1, 8): 1, (1, 257): 1, (64, 320): 1, (1, 1024): 1, (1, 1025): 2, (1, 4096): 4, (3, 4097): 5, (64, 5000): 5,
              (1, 128256): 64, (8, 128256): 64, (9, 128256): 57, (64, 128256): 8, (1, 151936): 64, (64, 151936): 8, (1, 65537): 64,
              (2, 300000): 64, (0, 100): 0, (65, 100): 0, (1, 0): 0}


def test_the_slab_rule_against_the_hand_table():
    for (rows, vocab), want in SLAB_TABLE.items():
        assert ops.token_logprob_slabs(rows, vocab) == want, (rows, vocab)
        if want:
            assert R.slabs(rows, vocab) == want, (rows, vocab)
            assert R.slab_len(rows, vocab) % 4 == 0 and (want - 1) * R.slab_len(rows, vocab) < vocab <= want * R.slab_len(rows, vocab)
    for rows in (1, 2, 7, 8, 9, 31, 64):
        for vocab in (1, 5, 1023, 2048, 2049, 32000, 50257, 128256, 151936):
            s = ops.token_logprob_slabs(rows, vocab)
            assert s == R.slabs(rows, vocab) and 1 <= s <= 64, (rows, vocab)
