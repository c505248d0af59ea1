"""The scoring surface of the C ABI without a GPU: the new symbols are exported with the signatures the headers declare, the
entry points answer NULL handles and buffers as declared, and KjarniScoreResult has the declared layout (mirrors
tests/test_lanes_abi.py)."""
import ctypes as C
import os
import re

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SCORE_SYMBOLS = {
    "kjarni_hip_decoder_score": 7, "kjarni_hip_decoder_set_score_fused": 2, "kjarni_hip_decoder_score_calls": 3,
    "kjarni_hip_op_score_head": 14, "kjarni_generator_score": 4,
}


def _declarations():
    text = ""
    for h in ("kjarni.h", "kjarni_hip.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_score_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in SCORE_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/*.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    assert _ffi.SIGNATURES["kjarni_hip_decoder_score_calls"][0] is None
    assert _ffi.SIGNATURES["kjarni_hip_decoder_set_score_fused"][0] is None
    assert _ffi.SIGNATURES["kjarni_hip_decoder_score"][0] is C.c_int32


def test_null_handles_and_buffers_write_nothing():
    ids = (C.c_uint32 * 3)(5, 6, 7)
    lp, tlp, lse = (C.c_float * 2)(9.0, 9.0), (C.c_float * 2)(9.0, 9.0), (C.c_float * 2)(9.0, 9.0)
    top = (C.c_uint32 * 2)(9, 9)
    assert L.kjarni_hip_decoder_score(None, ids, 3, 1, lp, top, tlp) == E.NULL_POINTER
    x = (C.c_float * 64)()
    tg = (C.c_uint32 * 2)(0, 1)
    assert L.kjarni_hip_op_score_head(0, None, 2, 32, None, 0, 64, None, 0, 1, lp, top, tlp, lse) == E.NULL_POINTER
    assert L.kjarni_hip_op_score_head(0, x, 2, 32, None, 0, 64, tg, 0, 1, lp, top, tlp, lse) == E.NULL_POINTER
    assert L.kjarni_hip_op_score_head(0, x, 2, 32, C.cast(x, C.c_void_p), 0, 64, None, 0, 0, lp, top, tlp, lse) == E.NULL_POINTER
    r = _ffi.KjarniScoreResult(7.0, 7, 7)
    assert L.kjarni_generator_score(None, b"a", b"b", C.byref(r)) == E.NULL_POINTER
    assert (r.sum_logprob, r.n_tokens, r.is_greedy) == (7.0, 7, 7)
    assert list(lp) == list(tlp) == list(lse) == [9.0, 9.0] and list(top) == [9, 9]     # nothing written
    L.kjarni_hip_decoder_set_score_fused(None, 0)                                      # a NULL handle is ignored


def test_counters_answer_zeros_on_null():
    a, b = C.c_uint64(9), C.c_uint64(9)
    L.kjarni_hip_decoder_score_calls(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    L.kjarni_hip_decoder_score_calls(None, None, None)


def test_score_result_layout():
    R = _ffi.KjarniScoreResult
    assert C.sizeof(R) == 24
    assert (R.sum_logprob.offset, R.n_tokens.offset, R.is_greedy.offset) == (0, 8, 16)
    assert (R.sum_logprob.size, R.n_tokens.size, R.is_greedy.size) == (8, 8, 4)
    # the header's declaration, field by field
    text = open(os.path.join(ROOT, "include", "kjarni.h")).read()
    m = re.search(r"typedef struct KjarniScoreResult \{([^}]*)\} KjarniScoreResult;", text)
    assert m and [f.strip() for f in m.group(1).split(";") if f.strip()] == ["double sum_logprob", "size_t n_tokens", "int32_t is_greedy"]
