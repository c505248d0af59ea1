"""The top-k scoring surface of the C ABI without a GPU (mirrors tests/test_score_abi.py): the new symbols are declared in the
headers, exported and bound with the declared arity; NULL handles answer NULL_POINTER and write nothing; KjarniTokenScores
has the declared layout; kjarni_token_scores_free takes NULL and a zeroed struct."""
import ctypes as C
import os
import re

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

TOPK_SYMBOLS = {
    "kjarni_hip_decoder_score_topk": 8, "kjarni_hip_op_score_head_topk": 15, "kjarni_generator_score_tokens": 5,
    "kjarni_token_scores_free": 1,
}
FIELDS = ["uint32_t* tokens", "float* logprobs", "uint32_t* top_tokens", "float* top_logprobs", "size_t n_tokens", "size_t top_k"]


def _headers():
    return {h: open(os.path.join(ROOT, "include", h)).read() for h in ("kjarni.h", "kjarni_hip.h")}


def _declarations():
    text = "".join(re.sub(r"/\*.*?\*/", "", t, flags=re.S) for t in _headers().values())
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_topk_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in TOPK_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/*.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    assert _ffi.SIGNATURES["kjarni_token_scores_free"][0] is None
    for name in ("kjarni_hip_decoder_score_topk", "kjarni_hip_op_score_head_topk", "kjarni_generator_score_tokens"):
        assert _ffi.SIGNATURES[name][0] is C.c_int32
    m = re.search(r"#define KJARNI_SCORE_TOPK_MAX (\d+)", _headers()["kjarni_hip.h"])
    assert m and int(m.group(1)) == 8


def test_null_handles_and_buffers_write_nothing():
    ids = (C.c_uint32 * 3)(5, 6, 7)
    lp, lse = (C.c_float * 2)(9.0, 9.0), (C.c_float * 2)(9.0, 9.0)
    tid, tlp = (C.c_uint32 * 4)(9, 9, 9, 9), (C.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    assert L.kjarni_hip_decoder_score_topk(None, ids, 3, 1, 2, lp, tid, tlp) == E.NULL_POINTER
    x = (C.c_float * 64)()
    w = C.cast(x, C.c_void_p)
    tg = (C.c_uint32 * 2)(0, 1)
    assert L.kjarni_hip_op_score_head_topk(0, None, 2, 32, None, 0, 64, None, 0, 1, 2, lp, tid, tlp, lse) == E.NULL_POINTER
    assert L.kjarni_hip_op_score_head_topk(0, x, 2, 32, None, 0, 64, tg, 0, 1, 2, lp, tid, tlp, lse) == E.NULL_POINTER
    assert L.kjarni_hip_op_score_head_topk(0, x, 2, 32, w, 0, 64, None, 0, 0, 2, lp, tid, tlp, lse) == E.NULL_POINTER
    assert L.kjarni_hip_op_score_head_topk(0, None, 2, 32, w, 0, 64, tg, 0, 1, 2, lp, tid, tlp, lse) == E.NULL_POINTER
    sentinel = (C.c_uint32 * 1)(7)
    r = _ffi.KjarniTokenScores(sentinel, None, sentinel, None, 7, 7)
    assert L.kjarni_generator_score_tokens(None, b"a", b"b", 2, C.byref(r)) == E.NULL_POINTER
    assert (r.n_tokens, r.top_k, r.tokens[0], r.top_tokens[0]) == (7, 7, 7, 7) and not r.logprobs and not r.top_logprobs
    assert L.kjarni_generator_score_tokens(None, b"a", b"b", 2, None) == E.NULL_POINTER
    assert list(lp) == list(lse) == [9.0, 9.0] and list(tid) == [9] * 4 and list(tlp) == [9.0] * 4     # nothing written


def test_token_scores_layout():
    R = _ffi.KjarniTokenScores
    assert C.sizeof(R) == 48
    names = ["tokens", "logprobs", "top_tokens", "top_logprobs", "n_tokens", "top_k"]
    assert [f[0] for f in R._fields_] == names
    assert [getattr(R, n).offset for n in names] == [0, 8, 16, 24, 32, 40]
    assert [getattr(R, n).size for n in names] == [8] * 6
    # the header's declaration, field by field
    m = re.search(r"typedef struct KjarniTokenScores \{([^}]*)\} KjarniTokenScores;", _headers()["kjarni.h"])
    assert m and [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == FIELDS


def test_free_accepts_null_and_a_zeroed_struct():
    L.kjarni_token_scores_free(None)
    r = _ffi.KjarniTokenScores()
    L.kjarni_token_scores_free(C.byref(r))
    L.kjarni_token_scores_free(C.byref(r))                                               # and once more: still zeroed
    assert not r.tokens and not r.logprobs and not r.top_tokens and not r.top_logprobs and (r.n_tokens, r.top_k) == (0, 0)
