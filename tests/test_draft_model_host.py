"""Speculative decoding with a draft model, host side (no GPU): the new symbols, their arities and what they do with NULL
handles, the `_ffi` mirror against the header, and the round simulation of tests/draft_cases.py on hand-written cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from tests import draft_cases as DC

SYMBOLS = {"kjarni_hip_decoder_generate_draft": 12, "kjarni_hip_decoder_draft_round": 8, "kjarni_hip_generator_set_draft_model": 3,
           "kjarni_hip_chat_set_draft_model": 3, "kjarni_hip_chat_verify_gemv_calls": 3}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kjarni_hip.h")


def test_symbols_and_arities():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    for name in ("generate_draft", "draft_round"):
        assert callable(getattr(kjarni_amd.HipDecoder, name))
    assert callable(kjarni_amd.Generator.set_draft_model) and callable(kjarni_amd.Chat.set_draft_model)
    assert callable(kjarni_amd.Chat.verify_gemv_calls)


def test_the_header_declares_what_ffi_mirrors():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, argc in SYMBOLS.items():
        m = re.search(r"\b(\w[\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in kjarni_hip.h"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == argc, name
        returns_code = "KjarniErrorCode" in m.group(1)
        assert (_ffi.SIGNATURES[name][0] is C.c_int32) == returns_code, name
    # draft_tokens is a required plain argument of the token-level entry point: no struct carries a default for it
    m = re.search(r"kjarni_hip_decoder_generate_draft\s*\(([^)]*)\)", text)
    assert re.search(r"int32_t\s+draft_tokens", m.group(1))


def test_null_handles():
    L = kjarni_amd.lib()
    o = _ffi.KjarniHipSamplingOptions()
    o.max_new_tokens, o.repetition_penalty = 4, 1.0
    p = np.array([5, 6, 7], np.uint32)
    out = np.zeros(4, np.uint32)
    n = C.c_size_t(7)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    cb = _ffi.KjarniTokenCallbackFn()
    assert L.kjarni_hip_decoder_generate_draft(None, None, u32(p), 3, C.byref(o), 4, cb, None, u32(out), 4, C.byref(n), None) == E.NULL_POINTER
    assert n.value == 0
    assert L.kjarni_hip_decoder_generate_draft(None, None, u32(p), 3, None, 4, cb, None, u32(out), 4, C.byref(n), None) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_generate_draft(None, None, u32(p), 3, C.byref(o), 4, cb, None, u32(out), 4, None, None) == E.NULL_POINTER
    # the options are judged on their own, ahead of the handles (as kjarni_hip_decoder_generate_sampled)
    u = np.zeros(2, np.float32)
    o.uniforms, o.n_uniforms = u.ctypes.data_as(C.POINTER(C.c_float)), 2
    assert L.kjarni_hip_decoder_generate_draft(None, None, u32(p), 3, C.byref(o), 4, cb, None, u32(out), 4, C.byref(n), None) == E.INVALID_CONFIG
    a = C.c_int32(0)
    picks, draft = np.zeros(8, np.uint32), np.zeros(7, np.uint32)
    assert L.kjarni_hip_decoder_draft_round(None, None, 5, 4, u32(draft), u32(picks), C.byref(a), None) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_draft_model(None, b"x", 4) == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_draft_model(None, None, 0) == E.NULL_POINTER
    s, f = C.c_uint64(9), C.c_uint64(9)
    L.kjarni_hip_chat_verify_gemv_calls(None, C.byref(s), C.byref(f))
    assert (s.value, f.value) == (0, 0)


# ---- the simulation ----------------------------------------------------------------------------------------------------------

PROMPT = [11, 12, 13]
OUT = list(range(100, 120))            # 20 tokens: the first from the prompt's logits, 19 from rounds
SEQ = PROMPT + OUT


def test_simulate_all_accepted():
    for k in range(1, 8):
        log, gap = DC.simulate(OUT, DC.table_drafter(SEQ), PROMPT, k)
        assert gap == float("inf")
        assert all(m == k for m, _ in log)
        assert all(a == k for _, a in log[:-1])                               # every round but the last accepts its whole draft
        assert sum(a + 1 for _, a in log[:-1]) + log[-1][1] + 1 >= 19 > sum(a + 1 for _, a in log[:-1])
        assert len(log) == -(-19 // (k + 1))


def test_simulate_none_accepted():
    for k in (1, 4, 7):
        log, _ = DC.simulate(OUT, DC.table_drafter(SEQ, wrong_at=range(len(SEQ))), PROMPT, k)
        assert log == [(k, 0)] * 19                                            # one token per round


@pytest.mark.parametrize("k", [1, 4, 7])
def test_simulate_first_mismatch_at_each_position(k):
    for j in range(k):
        # the first round drafts the tokens at absolute positions 4 .. 4 + k - 1; the one at 4 + j is wrong
        log, _ = DC.simulate(OUT, DC.table_drafter(SEQ, wrong_at=[len(PROMPT) + 1 + j]), PROMPT, k)
        assert log[0] == (k, j)
        # the round after starts behind the correction and, the table being right everywhere else, accepts everything
        assert all(a == k for _, a in log[1:-1])
        assert sum(a + 1 for _, a in log[:-1]) < 19 <= sum(a + 1 for _, a in log[:-1]) + k + 1


def test_simulate_edges():
    assert DC.simulate([], DC.table_drafter(SEQ), PROMPT, 4) == ([], float("inf"))
    assert DC.simulate(OUT[:1], DC.table_drafter(SEQ), PROMPT, 4) == ([], float("inf"))  # the first token needs no round
    # an output that ends inside a draft: the last a is what the output confirms
    log, _ = DC.simulate(OUT[:4], DC.table_drafter(SEQ), PROMPT, 7)
    assert log == [(7, 3)]


class _ToyModel:
    """logits(ids, cache): row i prefers (sum of the tokens so far) % vocab by 1.0, the runner-up by 0.25 less."""
    vocab = 17

    def new(self):
        return []

    def logits(self, ids, cache):
        rows = []
        for t in ids:
            cache.append(int(t))
            row = np.zeros(self.vocab)
            best = sum(cache) % self.vocab
            row[best], row[(best + 1) % self.vocab] = 1.0, 0.75
            rows.append(row)
        return np.stack(rows)


def test_model_drafter_continues_greedily_and_reuses_its_prefix():
    m = _ToyModel()
    d = DC.ModelDrafter(m, lambda cache, keep: cache[:keep])
    hist = [3, 4]
    toks, gap = d(hist, 3)
    want, run = [], list(hist)
    for _ in range(3):
        want.append(sum(run) % 17)
        run.append(want[-1])
    assert toks == want and gap == pytest.approx(0.25)
    # a history that follows the draft for one token and then departs from it
    hist2 = hist + [want[0], 9]
    toks2, _ = d(hist2, 2)
    run = list(hist2)
    want2 = []
    for _ in range(2):
        want2.append(sum(run) % 17)
        run.append(want2[-1])
    assert toks2 == want2
