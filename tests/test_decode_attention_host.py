"""The decode-attention entry points without a GPU: the three symbols are declared, exported and bound with their arity, answer
NULL as declared, and refuse what the launchers refuse -- INVALID_CONFIG from the argument check, which comes before any GPU
work, with the output buffers untouched.  Also the float64 reference against itself: the softmax over all keys equals the
merge of per-range slabs, so tests/decode_attention_ref64.py's two halves agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import decode_attention_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {"kjarni_hip_op_decode_attention": 26, "kjarni_hip_op_gemv_row_att": 12, "kjarni_hip_op_llm_gemv_att": 12}


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/kjarni_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is C.c_int32
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name


def test_null_pointers():
    f = (C.c_float * 4096)()
    i = (C.c_int32 * 8)()
    A = L.kjarni_hip_op_decode_attention
    args = [0, f, 64, 1, f, 4096, 64, f, 4096, 64, 4, 0, 0, 1, 64, -1, 1, 1, 0, 0, 0, None, None, f, 64, None]
    for at in (1, 4, 7, 23):                                             # q, k, v, ctx
        bad = list(args)
        bad[at] = None
        assert A(*bad) == E.NULL_POINTER
    G = L.kjarni_hip_op_gemv_row_att
    args = [0, f, 1, 64, f, None, f, 1, 512, 0, 0, f]
    for at in (1, 4, 11):                                                # slabs, w, y
        bad = list(args)
        bad[at] = None
        assert G(*bad) == E.NULL_POINTER
    M = L.kjarni_hip_op_llm_gemv_att
    args = [0, f, 1, 64, C.cast(f, C.c_void_p), 0, None, f, 1, 2048, 1, f]
    for at in (1, 4, 11):
        bad = list(args)
        bad[at] = None
        assert M(*bad) == E.NULL_POINTER
    assert list(i) == [0] * 8 and not any(f)


# ---- refusals: the argument check comes first, so none of these needs a device ----------------------------------------------------------

def _attention(n=8, heads=1, d=64, splits=1, rows=1, **kw):
    """A call with valid buffers for `n` keys (zeros: nothing may read them); the output starts as 7.0 and must stay so."""
    q = np.zeros((rows, heads * d), np.float32)
    kv = np.zeros(rows * max(n, 1) * heads * d, np.float32)
    ctx = np.full((rows, heads * d), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(_ffi._f32p)  # noqa: E731
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    pos, live = kw.get("lane_pos"), kw.get("lane_live")
    keep = [ip(pos), ip(live)]
    rc = L.kjarni_hip_op_decode_attention(0, p(q), heads * d, rows, p(kv), kv.size, heads * d, p(kv), kv.size, heads * d, n,
                                          int(kw.get("keys_on_device", 0)), int(kw.get("max_keys", 0)), heads, d, -1, splits, 1,
                                          int(kw.get("lane_stride", 0)), int(kw.get("lane_stride", 0)), int(kw.get("lanes", 0)), keep[0], keep[1],
                                          p(ctx), heads * d, None)
    assert rc == E.OK or (ctx == 7.0).all(), "a refused call wrote its output"
    return rc


@pytest.mark.parametrize("d", [12, 96, 256, 0, 2, -64])
def test_attention_refuses_head_dims_the_kernel_cannot_tile(d):
    """A key's lanes (head_dim / 4 of them) must tile the 256-thread workgroup, and a head fits 128 floats."""
    q = np.zeros((1, 1024), np.float32)
    kv = np.zeros(4096, np.float32)
    ctx = np.full((1, 1024), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(_ffi._f32p)  # noqa: E731
    rc = L.kjarni_hip_op_decode_attention(0, p(q), 1024, 1, p(kv), kv.size, 1024, p(kv), kv.size, 1024, 4, 0, 0, 1, d, -1, 1, 1, 0, 0, 0, None, None,
                                          p(ctx), 1024, None)
    assert rc == E.INVALID_CONFIG and b"launch_decode_attention refuses" in L.kjarni_last_error_message()
    assert (ctx == 7.0).all()


def test_attention_refuses_long_ranges_no_splits_and_bad_ragged_forms():
    assert _attention(n=513, splits=1) == E.INVALID_CONFIG                  # (n + splits - 1) / splits > 512
    assert _attention(n=1025, splits=2) == E.INVALID_CONFIG
    assert _attention(n=8, splits=0) == E.INVALID_CONFIG
    assert _attention(n=8, splits=-1) == E.INVALID_CONFIG
    assert _attention(n=8, rows=2, lanes=2, lane_stride=8 * 64, lane_pos=[1, 2]) == E.INVALID_CONFIG                       # ragged without lane_live
    assert _attention(n=8, rows=2, lanes=0, lane_stride=8 * 64, lane_pos=[1, 2], lane_live=[1, 1]) == E.INVALID_CONFIG      # ragged without lanes
    assert _attention(n=7, rows=2, lanes=2, lane_stride=8 * 64, lane_pos=[1, 2], lane_live=[1, 1], keys_on_device=1, max_keys=8) == E.INVALID_CONFIG
    assert _attention(n=600, splits=1, keys_on_device=1, max_keys=513) == E.INVALID_CONFIG   # with the device count, max_keys bounds the range
    for rc in (_attention(n=512, splits=1), _attention(n=1024, splits=2)):  # the largest ranges pass the check: only the device is missing
        assert rc == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


def test_attention_refuses_keys_outside_the_buffers():
    q = np.zeros((1, 64), np.float32)
    kv = np.zeros(8 * 64, np.float32)
    for kw in (dict(n_keys=9), dict(n_keys=8, ldk=68), dict(n_keys=7, keys_on_device=True, max_keys=7), dict(n_keys=8, ldk=62),
               dict(n_keys=4, k_lane_stride=2), dict(n_keys=0), dict(n_keys=8, kv_group=2)):
        args = dict(ldk=64, ldv=64, heads=1, head_dim=64, splits=1)
        n = kw.pop("n_keys")
        args.update(kw)
        with pytest.raises(KjarniException) as e:
            ops.decode_attention(q, kv, kv, n_keys=n, **args)
        assert e.value.code == E.INVALID_CONFIG, kw


def _projection(op, k, d, splits, residual=True, **kw):
    slabs = np.zeros((k // d, max(splits, 1), d + 4), np.float32)
    if splits != slabs.shape[1]:
        slabs = slabs[:, :0]
    w = np.zeros((6, k), np.float32)
    with pytest.raises(KjarniException) as e:
        op(slabs, w, None, np.zeros(6, np.float32) if residual else None, d, **kw)
    return e.value.code


def test_gemv_row_att_refuses():
    assert _projection(ops.gemv_row_att, 512, 64, 17) == E.INVALID_CONFIG
    assert _projection(ops.gemv_row_att, 2048, 64, 17) == E.INVALID_CONFIG
    assert _projection(ops.gemv_row_att, 1024, 64, 4) == E.INVALID_CONFIG
    assert _projection(ops.gemv_row_att, 512, 64, 4, residual=False) == E.INVALID_CONFIG
    assert _projection(ops.gemv_row_att, 512, 64, 0) == E.INVALID_CONFIG
    assert _projection(ops.gemv_row_att, 512, 2, 4) == E.INVALID_CONFIG       # head_dim no multiple of 4
    assert _projection(ops.gemv_row_att, 512, 64, 4, two_step=True, residual=False) == E.INVALID_CONFIG


def test_llm_gemv_att_refuses():
    assert _projection(ops.llm_gemv_att, 2048, 64, 9) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 4096, 128, 5) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 1024, 64, 4) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 2048, 64, 4, rows=2) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 2048, 64, 4, residual=False) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 8192, 128, 2) == E.INVALID_CONFIG
    assert _projection(ops.llm_gemv_att, 2048, 64, 0) == E.INVALID_CONFIG


# ---- the reference against itself ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("splits", [1, 3, 8])
def test_reference_softmax_equals_the_merge_of_its_ranges(splits):
    """attention64 never splits the keys; merge64 only merges.  Slabs cut from float64 scores, merged, must give attention64's
    row: the two halves of the reference describe the same function (masked and empty ranges included)."""
    rng = np.random.default_rng(splits)
    heads, d, n, base = 2, 16, 13, 9
    q = rng.standard_normal((1, heads * d)).astype(np.float32)
    k, v = (rng.standard_normal((n, heads * d)).astype(np.float32) for _ in range(2))
    ref = R.attention64(q, k, v, heads * d, heads * d, n, heads, d, causal_base=base)
    (sc,), _ = R.scores64(q, k, heads * d, n, heads, d, causal_base=base)
    chunk = (n + splits - 1) // splits
    slabs = np.zeros((heads, splits + 1, d + 4))
    slabs[:, splits, 0] = -np.inf                                        # one empty range behind the others
    for h in range(heads):
        for sp in range(splits):
            t0, t1 = sp * chunk, min(n, (sp + 1) * chunk)
            if t1 <= t0:
                slabs[h, sp, 0] = -np.inf
                continue
            m = sc[h, t0:t1].max()
            e = np.exp(sc[h, t0:t1] - m)
            slabs[h, sp, 0], slabs[h, sp, 1] = m, e.sum()
            slabs[h, sp, 4:] = e @ v[t0:t1, h * d:(h + 1) * d].astype(np.float64)
    assert np.abs(R.merge64(slabs) - ref[0]).max() < 1e-13
    w = rng.standard_normal((5, heads * d)).astype(np.float32)
    b, r = rng.standard_normal(5), rng.standard_normal(5)
    assert np.abs(R.merge_project64(slabs, w, b, r) - (w.astype(np.float64) @ ref[0] + b + r)).max() < 1e-12
    w16 = ops.to_bf16(w)
    assert np.array_equal(R.bf16_to_f64(w16), ops.bf16_to_f32(w16).astype(np.float64))
