"""The lanes surface of the C ABI without a GPU: the new symbols are exported with the signatures the headers declare,
and the entry points answer NULL handles and empty batches as declared (mirrors tests/test_abi.py)."""
import ctypes as C
import os
import re

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

LANE_SYMBOLS = {
    "kjarni_hip_decoder_generate_batch": 14, "kjarni_hip_decoder_lanes_begin": 3, "kjarni_hip_decoder_lane_prefill": 4,
    "kjarni_hip_decoder_lanes_step": 5, "kjarni_hip_decoder_lane_cache_len": 2, "kjarni_hip_decoder_lane_capacity": 1,
    "kjarni_hip_decoder_lane_kv_rows": 7, "kjarni_hip_decoder_lane_gemv_calls": 3, "kjarni_hip_generator_set_lanes": 2,
    "kjarni_generator_generate_batch": 5,
}


def _declarations():
    text = ""
    for h in ("kjarni.h", "kjarni_hip.h"):
        text += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_lane_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in LANE_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/*.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    assert _ffi.SIGNATURES["kjarni_hip_decoder_lane_gemv_calls"][0] is None
    assert _ffi.SIGNATURES["kjarni_hip_decoder_lane_cache_len"][0] is C.c_int32
    # the batch callback carries the prompt index in front of the token (by value), then the user pointer
    assert _ffi.KjarniBatchTokenCallbackFn._argtypes_ == (C.c_size_t, _ffi.KjarniToken, C.c_void_p)
    assert _ffi.KjarniBatchTokenCallbackFn._restype_ is C.c_bool


def test_null_handles_and_empty_batches():
    n_out = (C.c_size_t * 1)(7)
    off = (C.c_size_t * 2)(0, 1)
    new = (C.c_size_t * 1)(4)
    ids = (C.c_uint32 * 1)(5)
    cb = _ffi.KjarniBatchTokenCallbackFn()
    assert L.kjarni_hip_decoder_generate_batch(None, ids, off, 1, new, 1.0, 0, 0, 0, cb, None, None, 0, n_out) == E.NULL_POINTER
    assert n_out[0] == 7                                                 # nothing written
    assert L.kjarni_hip_decoder_lanes_begin(None, 8, 0) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_lane_prefill(None, 0, ids, 1) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_lanes_step(None, ids, None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_lane_cache_len(None, 0) == -1 and L.kjarni_hip_decoder_lane_capacity(None) == 0
    assert L.kjarni_hip_decoder_lane_kv_rows(None, 0, 0, 0, 0, None, None) == E.NULL_POINTER
    a, b = C.c_uint64(9), C.c_uint64(9)
    L.kjarni_hip_decoder_lane_gemv_calls(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    assert L.kjarni_hip_generator_set_lanes(None, 4) == E.NULL_POINTER
    arr = _ffi.KjarniStringArray()
    assert L.kjarni_generator_generate_batch(None, None, 0, None, C.byref(arr)) == E.NULL_POINTER
