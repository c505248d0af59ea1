"""The compact single-sequence KV cache without a GPU: the new symbols are exported and bound (tests/test_abi.py holds the bindings to
the header's declarations), NULL handles answer as declared, seq_attention_kv_accepts follows the header's rule, and the op hook
refuses before a device is asked for."""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E

L = kjarni_amd.lib()
SYMBOLS = {"kjarni_hip_decoder_set_kv_type": (2, C.c_int32), "kjarni_hip_decoder_kv_type": (1, C.c_int32),
           "kjarni_hip_decoder_cache_bytes": (1, C.c_uint64), "kjarni_hip_chat_set_kv_type": (2, C.c_int32),
           "kjarni_hip_generator_set_kv_type": (2, C.c_int32), "kjarni_hip_op_seq_attention_kv": (18, C.c_int32),
           "kjarni_hip_seq_attention_kv_accepts": (8, C.c_int32)}


def test_symbols_and_null_handles():
    for name, (arity, restype) in SYMBOLS.items():
        res, args = _ffi.SIGNATURES[name]
        assert hasattr(L, name) and len(args) == arity and res is restype, name
    from kjarni_amd import Chat, Generator, HipDecoder
    assert all(callable(getattr(cls, "set_kv_type")) for cls in (HipDecoder, Generator, Chat))
    assert callable(HipDecoder.cache_bytes) and callable(HipDecoder.kv_type) and callable(ops.seq_attention_kv)
    for fn in (L.kjarni_hip_decoder_set_kv_type, L.kjarni_hip_chat_set_kv_type, L.kjarni_hip_generator_set_kv_type):
        assert fn(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_kv_type(None) == 0 and L.kjarni_hip_decoder_cache_bytes(None) == 0


# (type, rows, base, capacity, heads, kv_heads, head_dim, splits) -> seq_attention_kv_accepts, written by hand from the header's rule
ACCEPTS = [((1, 1, 0, 1, 1, 1, 16, 1), 1), ((2, 130, 5, 135, 12, 1, 128, 3), 1), ((2, 130, 6, 135, 12, 1, 128, 3), 0), ((1, 0, 0, 8, 4, 4, 64, 1), 0),
           ((1, 8, -1, 64, 8, 2, 64, 1), 0), ((1, 8, 0, 64, 7, 2, 64, 1), 0), ((1, 8, 0, 64, 2, 4, 64, 1), 0), ((1, 8, 0, 64, 8, 2, 48, 1), 0),
           ((1, 8, 0, 64, 8, 2, 8, 1), 0), ((2, 8, 0, 64, 8, 2, 32, 4), 1), ((1, 8, 0, 64, 8, 2, 64, 0), 0), ((0, 8, 0, 64, 8, 2, 64, 1), 0),
           ((3, 8, 0, 64, 8, 2, 64, 1), 0)]


@pytest.mark.parametrize("args,want", ACCEPTS, ids=[",".join(map(str, a)) for a, _ in ACCEPTS])
def test_seq_attention_kv_accepts(args, want):
    assert L.kjarni_hip_seq_attention_kv_accepts(*args) == want


@pytest.mark.parametrize("change", [dict(kv_type=3), dict(d=48), dict(heads=7), dict(base=57), dict(splits=0), dict(scales=False)], ids=str)
def test_the_op_hook_refuses_before_any_gpu_work(change):
    c = dict(kv_type=2, heads=8, kv_heads=2, d=64, rows=8, cache=64, base=56, splits=1, scales=True)
    c.update(change)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    q = np.zeros((c["rows"], c["heads"] * c["d"] + 4), np.float32)
    codes = np.zeros((c["cache"], c["kv_heads"] * c["d"]), np.uint8)
    sc = np.zeros((c["cache"], c["kv_heads"]), np.float32)
    ctx = np.full((c["rows"], c["heads"] * c["d"]), 7.0, np.float32)
    rc = L.kjarni_hip_op_seq_attention_kv(0, c["kv_type"], f(q), q.shape[1], c["rows"], codes.ctypes.data, codes.ctypes.data,
                                          f(sc) if c["scales"] else None, f(sc) if c["scales"] else None, c["cache"], c["base"], c["heads"],
                                          c["kv_heads"], c["d"], c["splits"], f(ctx), ctx.shape[1], None)
    assert rc == E.INVALID_CONFIG and (ctx == 7.0).all()
