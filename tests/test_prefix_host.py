"""Prefix reuse without a GPU: the rule that says how many cache rows a call keeps (kjarni_hip_prefix_keep), and the new
surface of the C ABI -- every symbol declared in the headers, exported and bound with its arity, NULL handles and buffers
answered as declared (mirrors tests/test_score_abi.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

PREFIX_SYMBOLS = {
    "kjarni_hip_decoder_set_prefix_reuse": 2, "kjarni_hip_decoder_prefix_stats": 3, "kjarni_hip_decoder_resident": 4,
    "kjarni_hip_decoder_last_logits": 2,
    "kjarni_hip_prefix_keep": 6, "kjarni_hip_decoder_lane_prefill_shared": 5, "kjarni_hip_op_kv_prefix_copy": 10,
    "kjarni_hip_chat_set_prefix_reuse": 2, "kjarni_hip_chat_prefix_stats": 3,
    "kjarni_hip_generator_set_prefix_reuse": 2, "kjarni_hip_generator_prefix_stats": 3,
}

A = [11, 12, 13, 14, 15, 16, 17]
# (resident, prompt, limit, kept rows, what)
KEEP_TABLE = [
    ([], A, 6, 0, "an empty resident set"),
    (A, [], 0, 0, "an empty prompt"),
    (A, A, 6, 6, "identical sequences: the limit (the last prompt token is always forwarded)"),
    (A, A, 7, 7, "identical sequences, limit at the length"),
    (A, A, 100, 7, "a limit past both lengths"),
    (A, A[:4], 3, 3, "the prompt is a strict prefix of the resident set: limit n - 1"),
    (A, A[:4], 4, 4, "the prompt is a strict prefix of the resident set: all of the prompt"),
    (A[:4], A, 6, 4, "the resident set is a strict prefix of the prompt"),
    ([99] + A[1:], A, 6, 0, "divergence at index 0"),
    (A[:3] + [99] + A[4:], A, 6, 3, "divergence at index 3"),
    (A[:6] + [99], A, 6, 6, "divergence at the last index, limit before it"),
    (A[:6] + [99], A, 7, 6, "divergence at the last index, limit past it"),
    (A, A, 0, 0, "limit 0"),
    (A, A[:2] + [99] + A[3:], 1, 1, "the limit below the common prefix"),
    ([5], [5], 0, 0, "a one-token prompt keeps nothing"),
]


def _keep_python(resident, prompt, limit):
    n = 0
    while n < min(len(resident), len(prompt), limit) and resident[n] == prompt[n]:
        n += 1
    return n


@pytest.mark.parametrize("resident,prompt,limit,want,what", KEEP_TABLE, ids=[c[4] for c in KEEP_TABLE])
def test_prefix_keep_table(resident, prompt, limit, want, what):
    assert _keep_python(resident, prompt, limit) == want, "the table itself"
    assert kjarni_amd.prefix_keep(resident, prompt, limit) == want, what


def test_prefix_keep_equals_the_rule_on_random_sequences():
    rng = np.random.default_rng(0)
    for _ in range(300):
        a = rng.integers(0, 3, int(rng.integers(0, 12))).tolist()
        b = rng.integers(0, 3, int(rng.integers(0, 12))).tolist()
        limit = int(rng.integers(0, 14))
        assert kjarni_amd.prefix_keep(a, b, limit) == _keep_python(a, b, limit), (a, b, limit)


def _declarations():
    text = ""
    for h in ("kjarni.h", "kjarni_hip.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_prefix_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in PREFIX_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/*.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    for name in ("kjarni_hip_decoder_set_prefix_reuse", "kjarni_hip_decoder_prefix_stats", "kjarni_hip_chat_prefix_stats",
                 "kjarni_hip_generator_prefix_stats"):
        assert _ffi.SIGNATURES[name][0] is None, name
    for name in ("kjarni_hip_decoder_resident", "kjarni_hip_prefix_keep", "kjarni_hip_chat_set_prefix_reuse",
                 "kjarni_hip_generator_set_prefix_reuse", "kjarni_hip_decoder_lane_prefill_shared", "kjarni_hip_op_kv_prefix_copy"):
        assert _ffi.SIGNATURES[name][0] is C.c_int32, name
    # nothing of this lives in the reference-defined header
    ref_header = open(os.path.join(ROOT, "include", "kjarni.h")).read()
    assert "prefix_reuse" not in ref_header and "prefix_stats" not in ref_header


def test_python_surface():
    from kjarni_amd import Chat, Generator, HipDecoder
    for cls, names in ((HipDecoder, ("set_prefix_reuse", "prefix_stats", "resident", "lane_prefill_shared")),
                       (Chat, ("set_prefix_reuse", "prefix_stats")), (Generator, ("set_prefix_reuse", "prefix_stats"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls.__name__, n)
    from kjarni_amd import ops
    assert callable(kjarni_amd.prefix_keep) and callable(ops.kv_prefix_copy)


def test_null_handles_and_buffers():
    L.kjarni_hip_decoder_set_prefix_reuse(None, 1)                                      # a NULL handle is ignored
    for fn in (L.kjarni_hip_decoder_prefix_stats, L.kjarni_hip_chat_prefix_stats, L.kjarni_hip_generator_prefix_stats):
        a, b = C.c_uint64(9), C.c_uint64(9)
        fn(None, C.byref(a), C.byref(b))
        assert (a.value, b.value) == (0, 0)                                             # zeros on a NULL handle
        fn(None, None, None)                                                            # NULL outputs are allowed
        fn(None, C.byref(a), None)
    assert L.kjarni_hip_chat_set_prefix_reuse(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_prefix_reuse(None, 1) == E.NULL_POINTER
    out, n = (C.c_uint32 * 2)(9, 9), C.c_size_t(7)
    assert L.kjarni_hip_decoder_resident(None, out, 2, C.byref(n)) == E.NULL_POINTER
    assert list(out) == [9, 9] and n.value == 7                                         # nothing written
    ids = (C.c_uint32 * 3)(5, 6, 7)
    assert L.kjarni_hip_decoder_lane_prefill_shared(None, 0, 1, ids, 3) == E.NULL_POINTER
    x2 = (C.c_float * 2)(9.0, 9.0)
    assert L.kjarni_hip_decoder_last_logits(None, x2) == E.NULL_POINTER and list(x2) == [9.0, 9.0]
    keep = C.c_size_t(7)
    assert L.kjarni_hip_prefix_keep(ids, 3, ids, 3, 2, None) == E.NULL_POINTER
    assert L.kjarni_hip_prefix_keep(None, 3, ids, 3, 2, C.byref(keep)) == E.NULL_POINTER and keep.value == 7
    assert L.kjarni_hip_prefix_keep(ids, 3, None, 3, 2, C.byref(keep)) == E.NULL_POINTER and keep.value == 7
    assert L.kjarni_hip_prefix_keep(None, 0, None, 0, 5, C.byref(keep)) == E.OK and keep.value == 0   # empty sequences need no pointer
    x = (C.c_float * 8)()
    assert L.kjarni_hip_op_kv_prefix_copy(0, None, 1, 4, 0, 4, 0, 0, 4, x) == E.NULL_POINTER
    assert L.kjarni_hip_op_kv_prefix_copy(0, x, 1, 4, 0, 4, 0, 0, 4, None) == E.NULL_POINTER
