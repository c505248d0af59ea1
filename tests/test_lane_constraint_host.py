"""Constrained decoding in the lanes, host side (no GPU): the new symbols, their arities and what they do with NULL; the _ffi
mirror of the result struct and of the 8-lane state; every refusal of the two op hooks and of
kjarni_hip_decoder_generate_wide_constrained that needs no device, with the outputs untouched; the margins and the coverage counts
of tests/lane_constraint_cases.py in the float64 references."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd import constraints as K
from kjarni_amd._ffi import KjarniError as E
from tests import lane_constraint_cases as LCC

SYMBOLS = {
    "kjarni_hip_op_lane_automaton_apply": 17, "kjarni_hip_op_lane_automaton_pick": 22, "kjarni_hip_decoder_generate_wide_constrained": 21,
    "kjarni_hip_generator_batch_constraint_result": 3,
}
SEED_HOOK = "kjarni_hip_generator_batch_seed"       # (returns the seed itself, not an error code)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kjarni_hip.h")
RESULT_FIELDS = ["kind", "final_state", "device_state", "final_depth", "device_depth", "accepted", "complete", "violated"]

f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
u16 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint16))  # noqa: E731


def test_symbols_and_arities():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    assert callable(kjarni_amd.HipDecoder.generate_wide_constrained)
    assert callable(kjarni_amd.Generator.batch_constraint_result)
    assert callable(K.LaneAutomata) and callable(K.lane_result_dict)
    assert hasattr(L, SEED_HOOK) and len(_ffi.SIGNATURES[SEED_HOOK][1]) == 2 and _ffi.SIGNATURES[SEED_HOOK][0] is C.c_uint64
    assert L.kjarni_hip_generator_batch_seed(None, 0) == 0 and callable(kjarni_amd.Generator.batch_seed)


def test_the_header_declares_what_ffi_mirrors():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, argc in SYMBOLS.items():
        m = re.search(r"\b(\w[\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in kjarni_hip.h"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == argc, name
        assert "KjarniErrorCode" in m.group(1) and _ffi.SIGNATURES[name][0] is C.c_int32, name
    fields = [f for f, _ in _ffi.KjarniHipLaneAutomatonResult._fields_]
    assert fields == RESULT_FIELDS
    m = re.search(r"typedef struct KjarniHipLaneAutomatonResult \{(.*?)\}", text, re.S)
    assert [w for w in re.findall(r"\w+", m.group(1)) if w in fields] == fields
    assert C.sizeof(_ffi.KjarniHipLaneAutomatonResult) == 8 * 4
    # the 8-lane state: the wide state's fields, 8 entries each
    assert re.search(r"#define\s+KJARNI_HIP_BATCH_LANES\s+8\b", text)
    assert [f for f, _ in _ffi.KjarniHipLaneState._fields_] == [f for f, _ in _ffi.KjarniHipWideState._fields_]
    assert C.sizeof(_ffi.KjarniHipLaneState) == 8 * 4 * (6 + 16) and C.sizeof(_ffi.KjarniHipWideState) == 8 * C.sizeof(_ffi.KjarniHipLaneState)
    assert K.LANE_SLOTS == 64
    # the new entry is generate_wide_logprobs' argument list plus three arrays
    assert _ffi.SIGNATURES["kjarni_hip_decoder_generate_wide_constrained"][1][:18] == _ffi.SIGNATURES["kjarni_hip_decoder_generate_wide_logprobs"][1]
    assert "not constrained" not in open(HEADER).read()
    assert "not constrained" not in (kjarni_amd.Generator.set_constraint.__doc__ or "")


def _arrays():
    a = K.LaneAutomata([])
    return a


def _apply(L, logits, out, a, lanes=2, first=0, vocab=8, ld=8, live=None, skip=None):
    lv = np.ones(64, np.int32) if live is None else live
    args = [0, f32(logits), ld, vocab, lanes, first, i32(lv), i32(a.kinds), a.constraints, a.grammars, u32(a.states), i32(a.depths),
            u16(a.stacks), i32(a.done), u32(a.stops), i32(a.n_stop), f32(out)]
    if skip is not None:
        args[skip] = None
    return L.kjarni_hip_op_lane_automaton_apply(*args)


def test_lane_apply_hook_refuses_without_a_device():
    L = kjarni_amd.lib()
    logits, out = np.full((2, 8), 7.0, np.float32), np.full((2, 8), 9.0, np.float32)
    a = _arrays()
    for skip in (1, 6, 7, 10, 11, 12, 13, 14, 15, 16):                 # every array but the two handle arrays
        assert _apply(L, logits, out, a, skip=skip) == E.NULL_POINTER, skip
    for kw, word in ((dict(lanes=0), "lanes"), (dict(lanes=65), "lanes"), (dict(first=-1), "lanes"), (dict(first=63, lanes=2), "lanes"),
                     (dict(vocab=0), "vocab"), (dict(vocab=9), "vocab"), (dict(ld=(1 << 20) + 1), "ld")):
        assert _apply(L, logits, out, a, **kw) == E.INVALID_CONFIG, kw
        assert word in _ffi.last_error(), (kw, _ffi.last_error())
    a.kinds[1] = 3
    assert _apply(L, logits, out, a) == E.INVALID_CONFIG and "lane 1" in _ffi.last_error() and "kinds" in _ffi.last_error()
    a.kinds[1] = 1                                                     # a pattern lane without a constraint
    assert _apply(L, logits, out, a) == E.INVALID_CONFIG and "lane 1" in _ffi.last_error() and "constraints" in _ffi.last_error()
    a.kinds[1] = 2
    assert _apply(L, logits, out, a) == E.INVALID_CONFIG and "lane 1" in _ffi.last_error() and "grammars" in _ffi.last_error()
    a.kinds[1], a.n_stop[0] = 0, 17
    assert _apply(L, logits, out, a) == E.INVALID_CONFIG and "lane 0" in _ffi.last_error() and "n_stop" in _ffi.last_error()
    a.n_stop[0], a.n_stop[5] = 0, 99                                   # (a lane outside the range is not looked at)
    assert _apply(L, logits, out, a) in (E.GPU_UNAVAILABLE, E.OK)
    if kjarni_amd.device_count() < 1:
        assert (out == 9.0).all()


def _pick(L, wide, logits, state, hist, a, lanes=2, first=0, vocab=8, ld=8, stride=4, capacity=8, skip=None):
    args = [0, wide, f32(logits), ld, vocab, lanes, first, C.cast(C.byref(state), C.c_void_p), i32(hist), stride, capacity, 1, i32(a.kinds),
            a.constraints, a.grammars, u32(a.states), i32(a.depths), u16(a.stacks), i32(a.done), u32(a.stops), i32(a.n_stop), i32(a.violated)]
    if skip is not None:
        args[skip] = None
    return L.kjarni_hip_op_lane_automaton_pick(*args)


@pytest.mark.parametrize("wide", [0, 1])
def test_lane_pick_hook_refuses_without_a_device(wide):
    L = kjarni_amd.lib()
    rows = 64 if wide else 8
    logits = np.full((2, 8), 7.0, np.float32)
    st = _ffi.KjarniHipWideState() if wide else _ffi.KjarniHipLaneState()
    st.live[0] = st.live[1] = 1
    st.limit[0] = st.limit[1] = 4
    hist = np.full((rows, 4), -5, np.int32)
    a = _arrays()
    for skip in (2, 7, 8, 12, 15, 16, 17, 18, 19, 20, 21):
        assert _pick(L, wide, logits, st, hist, a, skip=skip) == E.NULL_POINTER, skip
    bad = [(dict(lanes=0), "lanes"), (dict(lanes=rows + 1), "lanes"), (dict(first=rows - 1, lanes=2), "lanes"), (dict(vocab=9), "vocab"),
           (dict(stride=0), "hist_stride"), (dict(capacity=-1), "capacity")]
    for kw, word in bad:
        assert _pick(L, wide, logits, st, hist, a, **kw) == E.INVALID_CONFIG, kw
        assert word in _ffi.last_error(), (kw, _ffi.last_error())
    st.n_stop[1] = 17
    assert _pick(L, wide, logits, st, hist, a) == E.INVALID_CONFIG and "n_stop[1]" in _ffi.last_error()
    st.n_stop[1], st.count[0] = 0, 4                                   # a live lane whose count is no entry of its history
    assert _pick(L, wide, logits, st, hist, a) == E.INVALID_CONFIG and "count[0]" in _ffi.last_error()
    st.count[0] = 0
    a.kinds[0] = 1
    assert _pick(L, wide, logits, st, hist, a) == E.INVALID_CONFIG and "lane 0" in _ffi.last_error()
    assert (hist == -5).all() and (a.violated == -7).all() and st.count[0] == 0 and st.live[0] == 1


def test_generate_wide_constrained_null_and_top_k():
    L = kjarni_amd.lib()
    gen = L.kjarni_hip_decoder_generate_wide_constrained
    p, off, news = np.array([5, 6, 7], np.uint32), (C.c_size_t * 2)(0, 3), (C.c_size_t * 1)(4)
    ids, cnt = np.full(4, 9, np.uint32), (C.c_size_t * 1)(7)
    res = (_ffi.KjarniHipLaneAutomatonResult * 1)()
    res[0].kind = 9
    cb = _ffi.KjarniBatchTokenCallbackFn()
    assert gen(None, u32(p), off, 1, news, 1.0, 0, 0, 0, cb, None, u32(ids), 4, cnt, -1, None, None, None, None, None, res) == E.NULL_POINTER
    assert cnt[0] == 7 and (ids == 9).all() and res[0].kind == 9
    for k in (-2, 9):                                                  # top_k is judged ahead of the handle; -1 means no records
        assert gen(None, u32(p), off, 1, news, 1.0, 0, 0, 0, cb, None, u32(ids), 4, cnt, k, None, None, None, None, None, res) == E.INVALID_CONFIG
        assert "top_k" in _ffi.last_error()
    assert cnt[0] == 7 and res[0].kind == 9
    r = _ffi.KjarniHipLaneAutomatonResult()
    assert L.kjarni_hip_generator_batch_constraint_result(None, 0, C.byref(r)) == E.NULL_POINTER
    assert K.lane_result_dict(r) == dict.fromkeys(RESULT_FIELDS, 0)


@pytest.mark.parametrize("case", sorted(LCC.SEEDS))
def test_the_case_set_clears_the_margins_and_reaches_every_ending(case):
    seed, cfg, t, ps, news = LCC.case_set(case)
    assert len(ps) == LCC.N_PROMPTS == 72 and min(news) >= 4 and max(news) <= 10
    assert [LCC.kind_of(i) for i in range(5)] == ["none", "choices", "integer", "brackets", "none"]
    stops = LCC.stops_of(cfg)
    assert stops, "the stop ids are present in every run"
    hosts = LCC.host_automata(LCC.tokens_of(case, cfg), stops)
    outs, infos = LCC.reference_runs(case, cfg, t, ps, news, hosts)
    assert len(outs) == len(infos) == 72                              # no prompt is left out
    cov = LCC.check(case, infos)
    print(case, "seed", seed, "ending -> (prompts, different steps):", cov)
    assert all(n >= 4 and steps >= 2 for n, steps in cov.values())
    # the constrained texts are what their automata say
    toks = LCC.tokens_of(case, cfg)
    for i, (ids, x) in enumerate(zip(outs, infos)):
        text = b"".join(toks[k] for k in ids)
        if x["kind"] == "choices" and x["complete"]:
            assert text.decode() in LCC.CHOICES, (i, text)
        if x["kind"] == "integer" and x["accepted"]:
            assert re.fullmatch(r"-?(?:0|[1-9][0-9]*)", text.decode()), (i, text)
        if x["kind"] == "brackets" and x["accepted"]:
            depth = 0
            for ch in text.decode():
                depth += 1 if ch in "([" else -1
                assert depth >= 0
            assert depth == 0 and text
