"""The prompt-lookup surface of the C ABI without a GPU: the new symbols are declared, exported and bound with their arity,
NULL handles answer as declared, and kjarni_lookup_draft -- the host restatement of the draft rule -- equals the normative
Python rule of tests/lookup_cases.py (mirrors tests/test_lanes_abi.py)."""
import ctypes as C
import os
import re

import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import lookup_cases as LK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

LOOKUP_SYMBOLS = {
    "kjarni_hip_lookup_config_default": 0, "kjarni_hip_decoder_generate_lookup": 13, "kjarni_hip_op_lookup_draft": 6,
    "kjarni_lookup_draft": 5, "kjarni_hip_decoder_verify_step": 8, "kjarni_hip_decoder_verify_gemv_calls": 3,
    "kjarni_hip_generator_set_prompt_lookup": 2, "kjarni_hip_generator_verify_gemv_calls": 3,
}


def _declarations():
    text = ""
    for h in ("kjarni.h", "kjarni_hip.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_lookup_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in LOOKUP_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/*.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    assert _ffi.SIGNATURES["kjarni_hip_decoder_verify_gemv_calls"][0] is None
    assert _ffi.SIGNATURES["kjarni_hip_lookup_config_default"][0] is _ffi.KjarniHipLookupConfig
    assert [f for f, _ in _ffi.KjarniHipLookupConfig._fields_] == ["draft_tokens", "ngram_max", "ngram_min"]
    assert C.sizeof(_ffi.KjarniHipLookupConfig) == 12 and C.sizeof(_ffi.KjarniHipLookupStats) == 32


def test_config_default_and_null_handles():
    c = L.kjarni_hip_lookup_config_default()
    assert (c.draft_tokens, c.ngram_max, c.ngram_min) == LK.DEFAULT == (7, 3, 1)
    ids = (C.c_uint32 * 8)(5, 6, 7)
    n_out = C.c_size_t(7)
    stats = _ffi.KjarniHipLookupStats(9, 9, 9, 9)
    cb = _ffi.KjarniTokenCallbackFn()
    assert L.kjarni_hip_decoder_generate_lookup(None, ids, 3, 4, None, 0, None, cb, None, None, 0, C.byref(n_out),
                                                C.byref(stats)) == E.NULL_POINTER
    assert n_out.value == 7 and stats.verify_steps == 9                  # nothing written
    acc = C.c_int32(7)
    assert L.kjarni_hip_decoder_verify_step(None, 5, ids, 2, 3, ids, C.byref(acc), None) == E.NULL_POINTER
    assert acc.value == 7
    a, b = C.c_uint64(9), C.c_uint64(9)
    L.kjarni_hip_decoder_verify_gemv_calls(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    assert L.kjarni_hip_generator_set_prompt_lookup(None, 7) == E.NULL_POINTER
    a, b = C.c_uint64(9), C.c_uint64(9)
    L.kjarni_hip_generator_verify_gemv_calls(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    n = C.c_int32(7)
    assert L.kjarni_lookup_draft(ids, 3, None, None, C.byref(n)) == E.NULL_POINTER and n.value == 7
    assert L.kjarni_hip_op_lookup_draft(0, ids, 3, None, None, C.byref(n)) == E.NULL_POINTER and n.value == 7


def test_host_rule_config_ranges_name_the_field():
    for kw, field in ((dict(draft_tokens=0), "draft_tokens"), (dict(draft_tokens=8), "draft_tokens"), (dict(ngram_max=0), "ngram_max"),
                      (dict(ngram_max=5), "ngram_max"), (dict(ngram_min=0), "ngram_min"), (dict(ngram_max=2, ngram_min=3), "ngram_min")):
        with pytest.raises(KjarniException, match=field) as e:
            ops.lookup_draft([1, 2, 1], device=None, **kw)
        assert e.value.code == E.INVALID_CONFIG
    # NULL config: the default
    out, n = (C.c_uint32 * 8)(), C.c_int32(0)
    T = [1, 2, 3, 4, 1, 2]
    assert L.kjarni_lookup_draft((C.c_uint32 * len(T))(*T), len(T), None, out, C.byref(n)) == E.OK
    assert list(out[:n.value]) == LK.lookup_draft(T, 3, 1, 7) == [3, 4, 1, 2]


def test_host_rule_equals_the_python_rule_on_seeded_histories():
    seen_cfg, drafted, lengths = set(), 0, set()
    for T, (D, hi, lo) in LK.histories():
        want = LK.lookup_draft(T, hi, lo, D)
        assert ops.lookup_draft(T, D, hi, lo, device=None) == want, (T, D, hi, lo)
        seen_cfg.add((D, hi, lo))
        drafted += bool(want)
        lengths.add(len(want))
    assert seen_cfg == set(LK.CONFIGS) and len(LK.CONFIGS) == 70
    assert drafted >= 500 and lengths == set(range(0, 8))              # the cases draft, at every length


@pytest.mark.parametrize("name, T, cfg", LK.EDGE_CASES, ids=[c[0] for c in LK.EDGE_CASES])
def test_host_rule_edge_cases(name, T, cfg):
    D, hi, lo = cfg
    want = LK.lookup_draft(T, hi, lo, D)
    assert ops.lookup_draft(T, D, hi, lo, device=None) == want
    expect = {"n = 1": [], "all tokens equal": [9] * 7, "no match": [], "the only match at e = 1": [1, 2, 4, 5, 3],
              "ngram_min longer than any match": [], "ngram_min met exactly": [9, 1, 2, 3],
              "longest continuation beats latest": [2, 1, 2, 1, 2, 1, 2], "longer match beats longer continuation": [1, 2, 3, 4, 5, 6, 8]}
    if name in expect:
        assert want == expect[name]


def test_simulate_counts_what_a_run_emits():
    # a periodic output after a periodic prompt: every step after the first accepts a full draft
    prompt, out = [1, 2, 3] * 4, ([1, 2, 3] * 11)[:32]
    log = LK.simulate(prompt, out)
    assert all(m == 7 for m, _ in log) and all(a == 7 for _, a in log[:-1])
    assert sum(a + 1 for _, a in log[:-1]) + log[-1][1] == len(out) - 1   # the output ends inside the last draft: a is a lower bound
    assert LK.simulate(prompt, []) == [] and LK.simulate(prompt, [5]) == []
    assert LK.simulate([1, 2, 3, 4], [9, 8, 7]) == [(0, 0), (0, 0)]    # nothing to draft from: one token per step
