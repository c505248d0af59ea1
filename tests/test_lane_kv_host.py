"""The compact lane KV caches without a GPU: the new symbols' declarations and NULL behaviour, and every refusal of the two op
hooks (kjarni_hip_op_lane_kv_scatter, kjarni_hip_op_lane_attention_kv) -- INVALID_CONFIG before a device is asked for (so also on
a host without one), with every output untouched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E

L = kjarni_amd.lib()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"kjarni_hip_decoder_set_lane_kv_type": (2, C.c_int32), "kjarni_hip_decoder_lane_kv_type": (1, C.c_int32),
           "kjarni_hip_decoder_lane_cache_bytes": (2, C.c_uint64), "kjarni_hip_chat_set_lane_kv_type": (2, C.c_int32),
           "kjarni_hip_generator_set_lane_kv_type": (2, C.c_int32), "kjarni_hip_op_lane_kv_scatter": (23, C.c_int32),
           "kjarni_hip_op_lane_attention_kv": (20, C.c_int32), "kjarni_hip_lane_attention_kv_accepts": (7, C.c_int32)}


def test_symbols_constants_and_null_handles():
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    for name, (arity, restype) in SYMBOLS.items():
        res, args = _ffi.SIGNATURES[name]
        assert hasattr(L, name) and len(args) == arity and res is restype, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    for name, value in (("F32", 0), ("BF16", 1), ("F8_E4M3", 2)):
        assert re.search(r"#define KJARNI_HIP_LANE_KV_%s %d\b" % (name, value), header)
    from kjarni_amd import Chat, Generator, HipDecoder
    assert all(callable(getattr(cls, "set_lane_kv_type")) for cls in (HipDecoder, Generator, Chat))
    assert (HipDecoder.LANE_KV_F32, HipDecoder.LANE_KV_BF16, HipDecoder.LANE_KV_F8_E4M3) == (0, 1, 2)
    assert callable(HipDecoder.lane_cache_bytes) and callable(ops.lane_kv_scatter) and callable(ops.lane_attention_kv)
    assert L.kjarni_hip_decoder_set_lane_kv_type(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_lane_kv_type(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_lane_kv_type(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_lane_kv_type(None) == 0 and L.kjarni_hip_decoder_lane_cache_bytes(None, 1) == 0


# (type, lanes, capacity, heads, kv_heads, head_dim, splits) -> lane_attention_kv_accepts, written by hand from the header's rule
ACCEPTS = [((1, 1, 1, 1, 1, 16, 1), 1), ((2, 64, 512, 32, 8, 64, 1), 1), ((2, 65, 512, 32, 8, 64, 1), 0), ((1, 0, 512, 32, 8, 64, 1), 0),
           ((1, 9, 513, 32, 8, 64, 1), 0), ((1, 9, 1024, 32, 8, 64, 2), 1), ((1, 9, 1025, 32, 8, 64, 2), 0), ((2, 9, 4096, 32, 8, 128, 8), 1),
           ((2, 9, 4097, 32, 8, 128, 8), 0), ((1, 9, 1537, 12, 1, 32, 3), 0), ((1, 9, 1536, 12, 1, 32, 3), 1), ((1, 9, 64, 7, 1, 64, 4), 1),
           ((1, 9, 64, 7, 2, 64, 4), 0), ((1, 9, 64, 2, 4, 64, 4), 0), ((1, 9, 64, 8, 0, 64, 4), 0), ((1, 9, 64, 8, 2, 48, 4), 0),
           ((1, 9, 64, 8, 2, 8, 4), 0), ((1, 9, 64, 8, 2, 256, 4), 0), ((1, 9, 64, 8, 2, 64, 0), 0), ((1, 9, 0, 8, 2, 64, 4), 0),
           ((0, 9, 64, 8, 2, 64, 4), 0), ((3, 9, 64, 8, 2, 64, 4), 0)]


@pytest.mark.parametrize("args,want", ACCEPTS, ids=[",".join(map(str, a)) for a, _ in ACCEPTS])
def test_lane_attention_kv_accepts(args, want):
    assert L.kjarni_hip_lane_attention_kv_accepts(*args) == want


# a valid call: 2 lanes, 4 query heads over 2 KV heads of 16, 8 rows per lane
GOOD = dict(kv_type=2, lanes=2, heads=4, kv_heads=2, d=16, rows=8, cap=8, ld=4 * 16 + 4 * 16, pos=(0, 3), live=(1, 1), rotate=1, splits=1,
            gamma="none", scales=True)
REFUSALS = [("type 0", dict(kv_type=0)), ("type 3", dict(kv_type=3)), ("no lanes", dict(lanes=0)), ("65 lanes", dict(lanes=65)),
            ("head_dim 24", dict(d=24)), ("head_dim 144", dict(d=144)), ("more kv heads than heads", dict(kv_heads=5)),
            ("lane rows below the capacity", dict(cap=9)), ("capacity 0", dict(cap=0)), ("FP8 without scales", dict(scales=False)),
            ("negative position", dict(pos=(0, -1)))]
SCATTER_REFUSALS = REFUSALS + [("ld short", dict(ld=127)), ("position outside the tables", dict(rows=16, cap=16, pos=(0, 9))), ("one gamma", dict(gamma="one")),
                               ("the Qwen3 form without rotation", dict(gamma="both", rotate=0))]
ATTENTION_REFUSALS = REFUSALS + [("head_dim 48", dict(d=48, ld=512)), ("heads no multiple of kv heads", dict(heads=3)), ("no split", dict(splits=0)),
                                 ("257 splits", dict(splits=257)), ("513 keys per split", dict(rows=513, cap=513)), ("ldq short", dict(ld=63))]


def _f(a):
    return a.ctypes.data_as(_ffi._f32p)


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _planes(c):
    dt = np.uint16 if c["kv_type"] == 1 else np.uint8
    lanes = max(c["lanes"], 1)
    codes = [np.full((lanes, c["rows"], c["kv_heads"] * c["d"]), 7, dt) for _ in range(2)]
    scales = [np.full((lanes, c["rows"], c["kv_heads"]), 0.5, np.float32) for _ in range(2)]
    pos, live = np.array(c["pos"], np.int32), np.array(c["live"], np.int32)
    return codes, scales, pos, live


@pytest.mark.parametrize("what,change", SCATTER_REFUSALS, ids=[w for w, _ in SCATTER_REFUSALS])
def test_scatter_hook_refusals(what, change):
    c = dict(GOOD, **change)
    codes, scales, pos, live = _planes(c)
    qkv = np.full((max(c["lanes"], 1), c["ld"]), 0.25, np.float32)
    table = np.ones((8, c["d"] // 2), np.float32)
    gamma = np.ones(c["d"], np.float32)
    keep = [a.copy() for a in [qkv] + codes + scales]
    sp = [_f(a) if c["scales"] else None for a in scales]
    rc = L.kjarni_hip_op_lane_kv_scatter(0, c["kv_type"], _f(qkv), c["ld"], c["lanes"], c["heads"], c["kv_heads"], c["d"],
                                         _f(gamma) if c["gamma"] != "none" else None,
                                         _f(gamma) if c["gamma"] == "both" else None, 1e-6,
                                         _f(table), _f(table), 8, codes[0].ctypes.data,
                                         codes[1].ctypes.data, sp[0], sp[1], c["rows"], c["cap"], _i(pos),
                                         _i(live), c["rotate"])
    assert rc == E.INVALID_CONFIG, what
    assert all(np.array_equal(a, b) for a, b in zip([qkv] + codes + scales, keep)), what


@pytest.mark.parametrize("what,change", ATTENTION_REFUSALS, ids=[w for w, _ in ATTENTION_REFUSALS])
def test_attention_hook_refusals(what, change):
    c = dict(dict(GOOD, ld=64), **change)
    codes, scales, pos, live = _planes(c)
    q = np.full((max(c["lanes"], 1), c["ld"]), 0.25, np.float32)
    ctx = np.full((max(c["lanes"], 1), max(c["ld"], 64)), 3.0, np.float32)
    sp = [_f(a) if c["scales"] else None for a in scales]
    rc = L.kjarni_hip_op_lane_attention_kv(0, c["kv_type"], _f(q), c["ld"], c["lanes"], codes[0].ctypes.data,
                                           codes[1].ctypes.data, sp[0], sp[1], c["rows"], c["cap"], c["heads"], c["kv_heads"], c["d"], c["splits"],
                                           _i(pos), _i(live),
                                           _f(ctx), ctx.shape[1], None)
    assert rc == E.INVALID_CONFIG, what
    assert (ctx == 3.0).all(), what


def test_null_arguments_and_the_valid_call_reaches_the_device():
    c = dict(GOOD, ld=64)
    codes, scales, pos, live = _planes(c)
    q = np.zeros((2, 64), np.float32)
    rc = L.kjarni_hip_op_lane_attention_kv(0, 2, _f(q), 64, 2, None, codes[1].ctypes.data, None, None, 8, 8, 4, 2, 16, 1,
                                           _i(pos), _i(live),
                                           _f(q), 64, None)
    assert rc == E.NULL_POINTER
    assert L.kjarni_hip_op_lane_kv_scatter(0, 2, None, 128, 2, 4, 2, 16, None, None, 0.0, None, None, 8, None, None, None, None, 8, 8, None, None,
                                           1) == E.NULL_POINTER
    if kjarni_amd.device_count() == 0:  # every check passed: the next thing the hook asks for is a device
        with pytest.raises(kjarni_amd.KjarniException) as ei:
            ops.lane_attention_kv(2, q, codes[0], codes[1], 4, 2, 16, 8, 1, pos, live, k_scale=scales[0], v_scale=scales[1])
        assert ei.value.code == E.GPU_UNAVAILABLE
