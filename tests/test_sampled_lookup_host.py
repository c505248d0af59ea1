"""Prompt-lookup decoding for sampled requests, host side (no GPU): the new symbols and the layout of the options struct, the
block decision lookup_accept_sampled against the float64 oracle of tests/sampled_lookup_cases.py, and the errors that are
reported before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from tests import sampled_lookup_cases as S

PARAMS = {"k40-p0.9-minp0.05": dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05),
          "p0.9-minp0.05": dict(temperature=0.6, top_p=0.9, min_p=0.05),
          "k5": dict(temperature=1.0, top_k=5)}
SYMBOLS = {"kjarni_hip_decoder_generate_sampled": 11, "kjarni_hip_decoder_verify_step_sampled": 13, "kjarni_hip_decoder_sampling_routes": 3,
           "kjarni_hip_op_sample_candidates_rows": 12, "kjarni_hip_op_repetition_penalty_rows": 10, "kjarni_lookup_accept_sampled": 14,
           "kjarni_hip_generator_set_prompt_lookup_sampling": 2, "kjarni_hip_chat_set_prompt_lookup_sampling": 2,
           "kjarni_hip_sampling_options_layout": 2}


def test_symbols_and_layout():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    for name in ("generate_sampled", "verify_step_sampled", "sampling_routes"):
        assert callable(getattr(kjarni_amd.HipDecoder, name))
    for name in ("sample_candidates_rows", "repetition_penalty_rows", "lookup_accept_sampled"):
        assert callable(getattr(ops, name))
    assert callable(kjarni_amd.Generator.set_prompt_lookup_sampling) and callable(kjarni_amd.Chat.set_prompt_lookup_sampling)
    O = _ffi.KjarniHipSamplingOptions
    want = (C.c_size_t * 14)()
    assert L.kjarni_hip_sampling_options_layout(want, 14) == 14
    names = [n for n, _ in O._fields_]
    assert names == ["max_new_tokens", "repetition_penalty", "no_repeat_ngram", "sample", "temperature", "top_k", "top_p", "min_p",
                     "stop_ids", "n_stop", "uniforms", "n_uniforms", "seed"]
    assert [C.sizeof(O)] + [getattr(O, n).offset for n in names] == list(want)


def _oracle_block(block, draft, uniforms, params):
    """The oracle's decision of a block: (picks, a, draws used)."""
    picks, a = [], 0
    last = min(len(draft), block.shape[0] - 1)
    for r in range(last + 1):
        ids, probs, slack = S.distribution(block[r], **params)
        assert slack >= 1.0                                                   # asserted again on what the test uses
        u = uniforms[len(picks)]
        assert S.draw_clearance(probs, u) >= S.u_margin(1.0, params["temperature"])
        picks.append(S.pick(ids, probs, u))
        a = r
        if r == last or picks[-1] != draft[r]:
            break
    return picks, a, len(picks)


@pytest.mark.parametrize("name", sorted(PARAMS))
@pytest.mark.parametrize("vocab", [257, 2049])
def test_lookup_accept_sampled_equals_the_oracle(vocab, name):
    params = PARAMS[name]
    f = {k: v for k, v in params.items()}
    blocks = redraws = seen_a = 0
    kinds = set()
    for rows in range(1, 9):
        for n_draft in sorted({0, 1, rows // 2, rows - 1, 7} - ({0} if rows > 1 else set())):
            last = min(n_draft, rows - 1)
            for a_want in sorted({0, last // 2, last}):
                block, draft, uniforms, picks, rd = S.accept_block(vocab, rows, n_draft, a_want, params, seed=1000 * vocab + 97 * rows + 11 * n_draft + a_want)
                blocks += rows
                redraws += rd
                want = _oracle_block(block, draft, uniforms, params)
                assert want == (picks, a_want, a_want + 1)
                # spare draws behind the ones that may be used: a decision that takes one too many shows in draws_used
                got = ops.lookup_accept_sampled(block, draft, uniforms + [0.5] * (last + 1 - len(uniforms)), **f)
                assert got == want, (rows, n_draft, a_want, got, want)
                kinds.add("none" if a_want == 0 and last > 0 else "all" if a_want == last and last > 0 else "some" if last > 0 else "no draft")
                seen_a += 1
                # a strided block gives the same decision
                wide = np.full((rows, vocab + 3), np.float32(99.0))
                wide[:, :vocab] = block
                assert ops.lookup_accept_sampled(wide, draft, uniforms + [0.5] * (last + 1 - len(uniforms)), vocab=vocab, **f) == want
    assert kinds == {"none", "all", "some", "no draft"} and seen_a >= 40
    assert redraws <= S.MAX_REDRAW_RATE * blocks, (redraws, blocks)


def test_a_short_draft_is_not_read_past_its_end():
    """rows = 8 with a draft of 2: row 2 is the last one decided.  The buffer behind the draft holds the token row 2 picks, so a
    decision that reads draft[2] would take it for accepted and go on to row 3 with a fourth draw."""
    params = PARAMS["k40-p0.9-minp0.05"]
    vocab, rows = 257, 8
    block, draft, uniforms, picks, _ = S.accept_block(vocab, rows, 7, 7, params, seed=5)
    assert len(picks) == 8 and draft == picks[:7]
    L = kjarni_amd.lib()
    d = np.asarray(draft, np.uint32)                                          # d[2] == picks[2]: what a read past the end would see
    u = np.asarray(uniforms, np.float32)
    out = np.zeros(8, np.uint32)
    a, used = C.c_int32(-1), C.c_int32(-1)
    f32, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = L.kjarni_lookup_accept_sampled(block.ctypes.data_as(f32), vocab, rows, vocab, d.ctypes.data_as(u32), 2, params["temperature"],
                                        params["top_k"], params["top_p"], params["min_p"], u.ctypes.data_as(f32), out.ctypes.data_as(u32),
                                        C.byref(a), C.byref(used))
    assert rc == 0 and (a.value, used.value) == (2, 3) and out[:3].tolist() == picks[:3] and not out[3:].any()


def test_errors_without_a_device():
    L = kjarni_amd.lib()
    ids = (C.c_uint32 * 3)(5, 6, 7)
    n_out = C.c_size_t(7)
    u = (C.c_float * 2)(0.5, 0.5)
    o = _ffi.KjarniHipSamplingOptions()
    o.max_new_tokens, o.repetition_penalty, o.sample, o.temperature, o.top_k, o.top_p, o.min_p = 4, 1.0, 1, 1.0, -1, -1.0, -1.0
    o.uniforms, o.n_uniforms = u, 2                                           # fewer draws than tokens asked for
    cb = _ffi.KjarniTokenCallbackFn()
    assert L.kjarni_hip_decoder_generate_sampled(None, ids, 3, C.byref(o), None, cb, None, None, 0, C.byref(n_out), None) == E.INVALID_CONFIG
    assert "n_uniforms" in kjarni_amd._ffi.last_error() and n_out.value == 0
    o.n_uniforms, o.max_new_tokens = 2, 2
    assert L.kjarni_hip_decoder_generate_sampled(None, ids, 3, C.byref(o), None, cb, None, None, 0, C.byref(n_out), None) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_generate_sampled(None, ids, 3, None, None, cb, None, None, 0, C.byref(n_out), None) == E.NULL_POINTER
    picks = (C.c_uint32 * 8)()
    a = C.c_int32(0)
    assert L.kjarni_hip_decoder_verify_step_sampled(None, 5, ids, 2, 3, C.byref(o), None, 0, u, picks, C.byref(a), None, None) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_prompt_lookup_sampling(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_prompt_lookup_sampling(None, 1) == E.NULL_POINTER
    block = np.zeros((2, 8), np.float32)
    with pytest.raises(_ffi.KjarniException) as e:                            # rows outside 1..8
        ops.lookup_accept_sampled(np.zeros((9, 8), np.float32), [1], [0.5] * 9)
    assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(_ffi.KjarniException) as e:                            # ld < vocab
        ops.lookup_accept_sampled(block, [1], [0.5, 0.5], vocab=9)
    assert e.value.code == E.INVALID_CONFIG
