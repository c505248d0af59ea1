"""The dense decode-projection entry points without a GPU: kjarni_hip_op_llm_gemv and kjarni_hip_op_llm_qkv_rope are declared,
exported and bound with their arity, answer NULL as declared, and refuse what their checks refuse -- INVALID_CONFIG from the
argument check, which comes before any GPU work, with every output still holding its sentinel.  Also the three route rules restated
in Python (tests/dense_proj_ref64.py) against a table worked out by hand from the launchers, and the float64 reference against
naive loops."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from tests import dense_proj_ref64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {"kjarni_hip_op_llm_gemv": 31, "kjarni_hip_op_llm_qkv_rope": 25}
SENTINEL = 7.0
PASSES = (E.OK, E.GPU_UNAVAILABLE)   # past the check: only the device may be missing


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


def _p(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _v(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- kjarni_hip_op_llm_gemv ---------------------------------------------------------------------------------------------------------------

def _gemv(rows=2, k=16, n_out=6, lanes=0, x_rows=None, ldx=None, gamma=False, beta=False, layernorm=0, gelu=0, w2=False, swiglu=0, bf16=0,
          residual=False, ldr=None, r_is_y0=0, seg_q=0, seg_kv=0, ldy0=None, ldy12=None, out_rows=(4, 6, 6), row_off=0, on_device=0,
          norm_out=False, null_y=None):
    """A call with valid zero buffers for the sizes given; every output starts as a sentinel that a refused call must leave alone.
    Returns the error code."""
    kk, nn = max(k, 1), max(n_out, 1)
    ldx = k if ldx is None else ldx
    cols0 = seg_q if seg_q > 0 else n_out
    ldy0 = cols0 if ldy0 is None else ldy0
    ldy12 = seg_kv if ldy12 is None else ldy12
    ldr = n_out if ldr is None else ldr
    x = np.ones((max(rows, 1) if x_rows is None else max(x_rows, 1), max(ldx, kk)), np.float32)
    w = np.zeros((nn, kk), np.uint16 if bf16 else np.float32)
    ys = [np.full((max(out_rows[i], 1), max(ld, c, 1)), SENTINEL, np.float32) for i, (ld, c) in
          enumerate(((ldy0, cols0), (ldy12, seg_kv), (ldy12, seg_kv)))]
    yp = (C.c_void_p * 3)(*[None if null_y == i else y.ctypes.data for i, y in enumerate(ys)])
    orows = (C.c_int32 * 3)(*out_rows)
    vec = np.ones(kk, np.float32)
    r = np.zeros((max(rows, 1), max(ldr, nn)), np.float32) if residual else None
    no = np.full(kk, SENTINEL, np.float32) if norm_out else None
    route = (C.c_int32 * 16)(*([-5] * 16))
    rc = L.kjarni_hip_op_llm_gemv(0, lanes, _p(x), max(rows, 1) if x_rows is None else x_rows, ldx, rows, _p(vec) if gamma else None,
                                  _p(vec) if beta else None, 1e-5, layernorm, gelu, _v(w), _v(w) if w2 else None, bf16, swiglu, None, _p(r), ldr,
                                  r_is_y0, n_out, k, seg_q, seg_kv, yp, orows, ldy0, ldy12, row_off, on_device, _p(no), route)
    if rc != E.OK:
        assert all((y == SENTINEL).all() for y in ys) and (no is None or (no == SENTINEL).all()), "a refused call wrote its output"
        assert list(route) == [-5] * 16, "a refused call wrote its route"
    return rc


SEG = dict(seg_q=2, seg_kv=2, n_out=6)


@pytest.mark.parametrize("kw", [
    dict(lanes=2), dict(lanes=-1),
    dict(rows=9), dict(rows=-1), dict(rows=3, x_rows=2), dict(x_rows=65),
    dict(k=12), dict(k=20, ldx=24), dict(k=0), dict(k=-8), dict(k=4), dict(k=(1 << 16) + 8),                 # k % 8, k < 8, the cap
    dict(n_out=0), dict(n_out=-3), dict(n_out=(1 << 17) + 1), dict(n_out=1 << 13, k=1 << 14),                  # n_out * k above 2^26
    dict(ldx=18), dict(ldx=22), dict(ldx=12), dict(ldx=8), dict(ldx=(1 << 18) + 4),                            # ldx % 4, ldx < k
    dict(ldy0=5), dict(ldy0=0), dict(residual=True, ldr=5), dict(residual=True, ldr=0),                        # ldy, ldr do not cover n_out
    dict(out_rows=(1, 6, 6)), dict(out_rows=(0, 6, 6)), dict(out_rows=(4097, 6, 6)), dict(null_y=0),
    dict(layernorm=1), dict(layernorm=1, gamma=True), dict(layernorm=1, beta=True),                              # LayerNorm needs both
    dict(layernorm=1, gamma=True, beta=True, residual=True), dict(layernorm=1, gamma=True, beta=True, r_is_y0=1),
    dict(layernorm=1, gamma=True, beta=True, swiglu=1, w2=True),
    dict(gelu=1), dict(gelu=1, gamma=True), dict(gelu=1, layernorm=1, gamma=True, beta=True, **SEG),
    dict(swiglu=1, gamma=True), dict(swiglu=1, w2=True), dict(swiglu=1, w2=True, gamma=True, residual=True),    # no w2, no gamma, a residual
    dict(swiglu=1, w2=True, gamma=True, r_is_y0=1),
    dict(residual=True, gamma=True), dict(r_is_y0=1, gamma=True), dict(residual=True, r_is_y0=1),
    dict(norm_out=True, rows=1, k=2048), dict(norm_out=True, rows=1, k=2040, gamma=True), dict(norm_out=True, rows=2, k=2048, gamma=True),
    dict(norm_out=True, rows=1, k=2048, gamma=True, seg_q=2, seg_kv=2, n_out=6),
    dict(norm_out=True, rows=1, k=2048, gamma=True, beta=True, layernorm=1),
    dict(seg_q=2, seg_kv=1, n_out=6), dict(seg_q=2, seg_kv=3, n_out=6), dict(seg_q=6, seg_kv=0, n_out=6), dict(seg_q=-2, seg_kv=4, n_out=6),
    dict(seg_q=0, seg_kv=3, n_out=6), dict(seg_kv=-1),
    dict(ldy12=1, **SEG), dict(ldy0=1, **SEG), dict(null_y=1, **SEG), dict(null_y=2, **SEG), dict(r_is_y0=1, **SEG),
    dict(row_off=-1, **SEG), dict(row_off=5, **SEG), dict(row_off=4, out_rows=(4, 6, 5), **SEG), dict(row_off=4, out_rows=(4, 5, 6), **SEG),
    dict(row_off=5, on_device=1, **SEG), dict(out_rows=(4, 0, 6), **SEG),
], ids=str)
def test_gemv_refuses(kw):
    assert _gemv(**kw) == E.INVALID_CONFIG, kw


def test_gemv_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(rows=0), dict(rows=8, out_rows=(8, 6, 6)), dict(rows=1, x_rows=64), dict(k=8), dict(ldx=20), dict(ldy0=9), dict(lanes=1),
               dict(lanes=1, k=512), dict(bf16=1), dict(gamma=True), dict(gamma=True, beta=True), dict(layernorm=1, gamma=True, beta=True),
               dict(layernorm=1, gelu=1, gamma=True, beta=True), dict(swiglu=1, w2=True, gamma=True), dict(w2=True), dict(residual=True),
               dict(residual=True, ldr=9), dict(r_is_y0=1), dict(r_is_y0=1, ldr=0, ldy0=9), dict(norm_out=True, rows=1, k=2048, gamma=True),
               dict(norm_out=True, rows=1, k=8192, gamma=True, swiglu=1, w2=True), dict(norm_out=True, rows=1, k=4096, gamma=True, lanes=1),
               dict(**SEG), dict(row_off=4, **SEG), dict(row_off=4, on_device=1, **SEG), dict(ldy12=5, ldy0=3, **SEG), dict(residual=True, **SEG),
               dict(gamma=True, rows=1, **SEG), dict(layernorm=1, gamma=True, beta=True, rows=1, **SEG), dict(n_out=1 << 17, k=512, rows=1),
               dict(n_out=1 << 12, k=1 << 14, rows=1), dict(out_rows=(4096, 6, 6))):
        assert _gemv(**kw) in PASSES, kw
    assert _gemv() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


def test_gemv_null_pointers():
    f = (C.c_float * 256)()
    yp, orows, route = (C.c_void_p * 3)(C.addressof(f), None, None), (C.c_int32 * 3)(4, 0, 0), (C.c_int32 * 16)(*([-5] * 16))
    args = [0, 0, f, 2, 16, 2, None, None, 0.0, 0, 0, C.cast(f, C.c_void_p), None, 0, 0, None, None, 0, 0, 6, 16, 0, 0, yp, orows, 6, 0, 0, 0, None,
            route]
    for at in (2, 11, 23, 24, 30):                                         # x, w, y, out_rows, route_out
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_llm_gemv(*bad) == E.NULL_POINTER
    assert list(route) == [-5] * 16 and not any(f)


# ---- kjarni_hip_op_llm_qkv_rope -----------------------------------------------------------------------------------------------------------

def _qkv(k=16, heads=2, kv=1, d=4, positions=5, pos=2, cache_rows=4, on_device=0, bf16=0, gamma=True, x=True, embed=False, table=None, vocab=3,
         x_raw=False, bias=False):
    kk, hh, kvh, dd = max(k, 1), max(heads, 1), max(kv, 1), max(d, 2)
    n = (hh + 2 * kvh) * dd
    wt = np.uint16 if bf16 else np.float32
    w = np.zeros((n, kk), wt)
    xa = np.ones(kk, np.float32) if x else None
    ga = np.ones(kk, np.float32) if gamma else None
    ta = np.zeros((max(vocab, 1), kk), wt) if (embed if table is None else table) else None
    ida = np.array([1], np.uint32) if embed else None
    tab = np.ones((max(positions, 1), dd // 2), np.float32)
    q = np.full(hh * dd, SENTINEL, np.float32)
    kc, vc = (np.full((max(cache_rows, 1), kvh * dd), SENTINEL, np.float32) for _ in range(2))
    xr = np.full(kk, SENTINEL, np.float32) if x_raw else None
    ba = np.zeros(n, np.float32) if bias else None
    route = (C.c_int32 * 3)(-5, -5, -5)
    rc = L.kjarni_hip_op_llm_qkv_rope(0, _p(xa), None if ida is None else ida.ctypes.data_as(_ffi._u32p), _v(ta), vocab, _p(ga), 1e-5, _v(w), bf16,
                                      _p(ba), k, heads, kv, d, _p(tab), _p(tab), positions, pos, on_device, _p(q), _p(kc), _p(vc), cache_rows,
                                      _p(xr), route)
    if rc != E.OK:
        assert (q == SENTINEL).all() and (kc == SENTINEL).all() and (vc == SENTINEL).all() and (xr is None or (xr == SENTINEL).all()), \
            "a refused call wrote its output"
        assert list(route) == [-5] * 3, "a refused call wrote its route"
    return rc


@pytest.mark.parametrize("kw", [
    dict(gamma=False), dict(gamma=False, k=2048),
    dict(k=12), dict(k=0), dict(k=-8), dict(k=8200), dict(k=16384),
    dict(d=3), dict(d=5), dict(d=0), dict(d=-2), dict(d=1026),
    dict(heads=0), dict(heads=257), dict(kv=0), dict(kv=3), dict(heads=256, kv=256, d=128, k=2048),            # elements above 2^26
    dict(pos=-1), dict(pos=5), dict(pos=4), dict(pos=4, positions=9), dict(pos=6, cache_rows=9), dict(positions=0), dict(cache_rows=0),
    dict(cache_rows=4097, positions=5000), dict(pos=5, on_device=1),
    dict(x=False), dict(x=True, embed=True, k=2048), dict(x=False, embed=True, k=2040), dict(x=False, embed=True, k=16),
    dict(x=False, embed=True, table=False, k=2048), dict(x=False, embed=True, vocab=0, k=2048), dict(x=False, embed=True, vocab=(1 << 17) + 1, k=8),
    dict(table=True), dict(x_raw=True),
], ids=str)
def test_qkv_rope_refuses(kw):
    assert _qkv(**kw) == E.INVALID_CONFIG, kw


def test_qkv_rope_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(k=8), dict(k=8192), dict(d=2), dict(heads=3, kv=1, d=6), dict(kv=2), dict(pos=0), dict(pos=3), dict(pos=4, positions=5, cache_rows=5),
               dict(pos=3, on_device=1), dict(pos=0, on_device=1), dict(positions=1, cache_rows=1, pos=0, on_device=1), dict(bf16=1), dict(bias=True),
               dict(x=False, embed=True, k=2048), dict(x=False, embed=True, k=4096, x_raw=True, bf16=1), dict(x=False, embed=True, k=2048, vocab=1)):
        assert _qkv(**kw) in PASSES, kw


def test_qkv_rope_null_pointers():
    f = (C.c_float * 256)()
    route = (C.c_int32 * 3)(-5, -5, -5)
    args = [0, f, None, None, 0, f, 0.0, C.cast(f, C.c_void_p), 0, None, 16, 2, 1, 4, f, f, 5, 2, 0, f, f, f, 4, None, route]
    for at in (7, 14, 15, 19, 20, 21, 24):                                 # w, cos_t, sin_t, q, k_cache, v_cache, route
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_llm_qkv_rope(*bad) == E.NULL_POINTER
    assert list(route) == [-5] * 3 and not any(f)


def test_wrappers_check_their_shapes():
    x, w, y = np.zeros((2, 16), np.float32), np.zeros((6, 16), np.float32), np.zeros((2, 6), np.float32)
    with pytest.raises(ValueError):
        ops.llm_gemv(x, w, 2, [y, y])
    with pytest.raises(ValueError):
        ops.llm_gemv(x, w, 2, [y], gamma=np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        ops.llm_gemv(x, w, 2, [y], w2=np.zeros((5, 16), np.float32))
    t = np.ones((4, 2), np.float32)
    with pytest.raises(ValueError):
        ops.llm_qkv_rope(np.zeros((15, 16), np.float32), np.ones(16), 2, 1, 4, t, t, 0, np.zeros(8), np.zeros((4, 4)), np.zeros((4, 4)), x=np.zeros(16))
    with pytest.raises(ValueError):
        ops.llm_qkv_rope(np.zeros((16, 16), np.float32), np.ones(16), 2, 1, 4, t, t, 0, np.zeros(8), np.zeros((4, 4)), np.zeros((4, 5)), x=np.zeros(16))


# ---- the route rules restated, against a table worked out by hand from launch_gemv_t / launch_gemv_lanes_t / launch_llm_qkv_rope --------

def _g(kernel, ch=0, wide=0, threads=256, loop=0, rpb=1, wgs=0):
    return dict(kernel=kernel, ch=ch, wide=wide, threads=threads, loop=loop, rows_per_batch=rpb, workgroups=wgs)


GEMV_TABLE = [
    # one row, streaming widths: the narrow form, the 16-load form from 2048 batches of 4 (bf16) or 2 (f32, SwiGLU) rows, the loop past 4096 batches
    (dict(rows=1, k=2048, n_out=1, bf16=True), _g(D.STREAM, 4, wgs=1)),
    (dict(rows=1, k=2048, n_out=1027, bf16=True), _g(D.STREAM, 4, wgs=257)),
    (dict(rows=1, k=2048, n_out=4096, bf16=True), _g(D.STREAM, 4, wgs=1024)),
    (dict(rows=1, k=2048, n_out=8191, bf16=True), _g(D.STREAM, 4, wide=1, loop=1, rpb=4, wgs=512)),     # 8191 one-row batches: already looping
    (dict(rows=1, k=2048, n_out=8192, bf16=True), _g(D.STREAM, 4, wide=1, rpb=4, wgs=512)),
    (dict(rows=1, k=2048, n_out=8195, bf16=True), _g(D.STREAM, 4, wide=1, rpb=4, wgs=513)),
    (dict(rows=1, k=2048, n_out=16384, bf16=True), _g(D.STREAM, 4, wide=1, rpb=4, wgs=1024)),
    (dict(rows=1, k=2048, n_out=16400, bf16=True), _g(D.STREAM, 4, wide=1, loop=1, rpb=4, wgs=512)),
    (dict(rows=1, k=2048, n_out=4095), _g(D.STREAM, 4, wgs=1024)),
    (dict(rows=1, k=2048, n_out=4096), _g(D.STREAM, 4, wide=1, rpb=2, wgs=512)),
    (dict(rows=1, k=2048, n_out=4099), _g(D.STREAM, 4, wide=1, rpb=2, wgs=513)),
    (dict(rows=1, k=2048, n_out=8192), _g(D.STREAM, 4, wide=1, rpb=2, wgs=1024)),
    (dict(rows=1, k=2048, n_out=8200), _g(D.STREAM, 4, wide=1, loop=1, rpb=2, wgs=512)),
    (dict(rows=1, k=2048, n_out=4096, bf16=True, swiglu=True, norm=True), _g(D.STREAM, 4, wide=1, rpb=2, wgs=512)),
    (dict(rows=1, k=2048, n_out=4096, swiglu=True, norm=True), _g(D.STREAM, 4, wide=1, wgs=1024)),      # f32 pair: 16 loads are one row
    (dict(rows=1, k=2048, n_out=2047, swiglu=True, norm=True), _g(D.STREAM, 4, wgs=512)),
    (dict(rows=1, k=4096, n_out=5, bf16=True), _g(D.STREAM, 8, wgs=2)),
    (dict(rows=1, k=4096, n_out=4096, bf16=True), _g(D.STREAM, 8, wide=1, rpb=2, wgs=512)),
    (dict(rows=1, k=8192, n_out=2047, bf16=True), _g(D.STREAM, 16, wgs=512)),
    (dict(rows=1, k=8192, n_out=2048, bf16=True), _g(D.STREAM, 16, wide=1, threads=512, wgs=256)),
    (dict(rows=1, k=8192, n_out=2051), _g(D.STREAM, 16, wide=1, threads=512, wgs=257)),
    (dict(rows=1, k=2048, n_out=2048, bf16=True, att_splits=4), _g(D.STREAM, 4, threads=512, wgs=256)),
    # one row, other widths: K over 4 waves in 1 / 2 / 4 chunks of 256 x 8 columns, over 16 waves from 8192
    (dict(rows=1, k=8, n_out=1), _g(D.SPLITK, 1, rpb=2, wgs=1)),
    (dict(rows=1, k=264, n_out=5), _g(D.SPLITK, 1, rpb=2, wgs=3)),
    (dict(rows=1, k=2040, n_out=2), _g(D.SPLITK, 1, rpb=2, wgs=1)),
    (dict(rows=1, k=2056, n_out=2, bf16=True), _g(D.SPLITK, 2, rpb=2, wgs=1)),
    (dict(rows=1, k=4088, n_out=5), _g(D.SPLITK, 2, rpb=2, wgs=3)),
    (dict(rows=1, k=4104, n_out=5), _g(D.SPLITK, 4, rpb=2, wgs=3)),
    (dict(rows=1, k=6144, n_out=5), _g(D.SPLITK, 4, rpb=2, wgs=3)),
    (dict(rows=1, k=8184, n_out=5, norm=True, swiglu=True), _g(D.SPLITK, 4, rpb=2, wgs=3)),
    (dict(rows=1, k=8200, n_out=5), _g(D.SPLITK, 2, wide=1, threads=1024, rpb=2, wgs=3)),
    (dict(rows=1, k=11008, n_out=1, bf16=True), _g(D.SPLITK, 2, wide=1, threads=1024, rpb=2, wgs=1)),
    (dict(rows=1, k=14336, n_out=2), _g(D.SPLITK, 2, wide=1, threads=1024, rpb=2, wgs=1)),
    (dict(rows=1, k=16384, n_out=2, norm=True), _g(D.SPLITK, 2, wide=1, threads=1024, rpb=2, wgs=1)),
    (dict(rows=1, k=768, n_out=5, layernorm=True, gelu_tanh=True, norm=True), _g(D.SPLITK, 1, rpb=2, wgs=3)),
    (dict(rows=1, k=2048, n_out=5, layernorm=True, gelu_tanh=True, norm=True), _g(D.SPLITK, 1, rpb=2, wgs=3)),
    # one row staged in LDS: LayerNorm Q | K | V, RMSNorm with segments
    (dict(rows=1, k=768, n_out=20, layernorm=True, norm=True, seg_q=8), _g(D.ONE, rpb=2, wgs=3)),
    (dict(rows=1, k=1600, n_out=9, layernorm=True, norm=True), _g(D.ONE, rpb=2, wgs=2)),
    (dict(rows=1, k=2048, n_out=9, layernorm=True, norm=True), _g(D.ONE, rpb=2, wgs=2)),
    (dict(rows=1, k=72, n_out=20, norm=True, seg_q=8), _g(D.ONE, rpb=2, wgs=3)),
    (dict(rows=1, k=2048, n_out=20, norm=True, seg_q=8), _g(D.ONE, rpb=2, wgs=3)),
    (dict(rows=1, k=16384, n_out=20, norm=True, seg_q=8), _g(D.ONE, rpb=2, wgs=3)),
    # everything else: a wave per column
    (dict(rows=1, k=16392, n_out=6, norm=True), _g(D.GENERIC, wgs=2)),
    (dict(rows=1, k=16392, n_out=6, norm=True, seg_q=2), _g(D.GENERIC, wgs=2)),
    (dict(rows=1, k=2048, n_out=20, seg_q=8), _g(D.GENERIC, wgs=5)),                                       # segments without a norm
    (dict(rows=1, k=4096, n_out=5, layernorm=True, gelu_tanh=True, norm=True), _g(D.GENERIC, wgs=2)),
    (dict(rows=2, k=2048, n_out=3, bf16=True), _g(D.GENERIC, wgs=1)),
    (dict(rows=8, k=768, n_out=6, layernorm=True, norm=True), _g(D.GENERIC, wgs=2)),
]


def _l(ch, ns, wide, cpw, wgs):
    return dict(taken=1, ch=ch, ns=ns, wide=wide, cpw=cpw, workgroups=wgs)


LANES_TABLE = [
    (dict(rows=2, k=504, n_out=7), dict(taken=0, ch=0, ns=0, wide=0, cpw=0, workgroups=0)),
    (dict(rows=1, k=2048, n_out=7, norm_out=True), dict(taken=0, ch=0, ns=0, wide=0, cpw=0, workgroups=0)),
    (dict(rows=1, k=512, n_out=1), _l(2, 1, 0, 1, 1)),
    (dict(rows=2, k=768, n_out=7), _l(2, 1, 0, 1, 2)),
    (dict(rows=5, k=1024, n_out=7, bf16=True), _l(2, 1, 0, 1, 2)),
    (dict(rows=8, k=520, n_out=7), _l(2, 1, 0, 1, 2)),            # 520 of 1024: the second 512-column piece is all but empty
    (dict(rows=2, k=1536, n_out=7), _l(4, 1, 0, 1, 2)),           # 1536 of 2048: the fourth piece is past K
    (dict(rows=2, k=2048, n_out=7), _l(4, 1, 0, 1, 2)),
    (dict(rows=2, k=2056, n_out=7), _l(2, 3, 0, 1, 2)),           # three 1024-column slices, the last with 8 columns
    (dict(rows=2, k=3072, n_out=7), _l(2, 3, 0, 1, 2)),
    (dict(rows=2, k=8192, n_out=7, bf16=True), _l(4, 4, 0, 1, 2)),
    (dict(rows=2, k=14336, n_out=7), _l(4, 7, 0, 1, 2)),
    (dict(rows=2, k=2048, n_out=2052, bf16=True), _l(4, 1, 0, 1, 512)),       # 513 batches on 512 workgroups
    (dict(rows=2, k=8192, n_out=2052, bf16=True), _l(4, 4, 0, 1, 513)),       # several slices: the grid covers the columns
    (dict(rows=2, k=2048, n_out=8176, bf16=True), _l(4, 1, 0, 1, 512)),
    (dict(rows=2, k=2048, n_out=8177, bf16=True), _l(4, 1, 1, 4, 512)),
    (dict(rows=2, k=2048, n_out=4088), _l(4, 1, 0, 1, 512)),
    (dict(rows=2, k=2048, n_out=4089), _l(4, 1, 1, 2, 512)),
    (dict(rows=2, k=2048, n_out=4089, bf16=True, swiglu=True), _l(4, 1, 1, 2, 512)),
    (dict(rows=2, k=1024, n_out=8177, bf16=True), _l(2, 1, 1, 4, 512)),       # CH = 2: 16 / 2 = 8 columns, clamped to 4
]

QKV_TABLE = [
    (dict(k=8, n_heads=3, n_kv_heads=1, head_dim=6), dict(kernel=D.PAIR, ch=1, workgroups=15)),
    (dict(k=264, n_heads=4, n_kv_heads=2, head_dim=64), dict(kernel=D.PAIR, ch=1, workgroups=256)),
    (dict(k=2040, n_heads=5, n_kv_heads=1, head_dim=32), dict(kernel=D.PAIR, ch=1, workgroups=112)),
    (dict(k=2056, n_heads=2, n_kv_heads=2, head_dim=80), dict(kernel=D.PAIR, ch=2, workgroups=240)),
    (dict(k=4104, n_heads=3, n_kv_heads=1, head_dim=6), dict(kernel=D.PAIR, ch=4, workgroups=15)),
    (dict(k=8184, n_heads=3, n_kv_heads=1, head_dim=6), dict(kernel=D.PAIR, ch=4, workgroups=15)),
    (dict(k=2048, n_heads=3, n_kv_heads=1, head_dim=6), dict(kernel=D.QKV_STREAM, ch=4, workgroups=4)),      # 15 pairs on 16 waves
    (dict(k=4096, n_heads=5, n_kv_heads=1, head_dim=32), dict(kernel=D.QKV_STREAM, ch=8, workgroups=28)),
    (dict(k=8192, n_heads=14, n_kv_heads=2, head_dim=128, embed=True), dict(kernel=D.QKV_STREAM_EMBED, ch=16, workgroups=288)),
]


def test_the_route_rules_restated_give_the_table():
    for kw, want in GEMV_TABLE:
        assert D.gemv_route(**kw) == want, kw
    for kw, want in LANES_TABLE:
        assert D.lanes_route(**kw) == want, kw
    for kw, want in QKV_TABLE:
        assert D.qkv_route(**kw) == want, kw
    assert {w["kernel"] for _, w in GEMV_TABLE} == {D.STREAM, D.SPLITK, D.ONE, D.GENERIC}
    assert {(w["ch"], w["threads"]) for _, w in GEMV_TABLE if w["kernel"] == D.SPLITK} == {(1, 256), (2, 256), (4, 256), (2, 1024)}
    # no K reaches the four-wave kernel's eight chunks: from 8192 on the sixteen-wave form has the row
    assert all(D.gemv_route(1, k, 4)["ch"] <= 4 for k in range(8, 16385, 8) if D.gemv_route(1, k, 4)["kernel"] == D.SPLITK)


# ---- the reference against naive loops ----------------------------------------------------------------------------------------------------

def test_gemv64_against_naive_loops():
    rng = np.random.default_rng(11)
    rows, n, k, eps = 3, 5, 16, 1e-5
    x, w, w2 = (rng.standard_normal(s).astype(np.float32) for s in ((rows, k), (n, k), (n, k)))
    gamma, beta, bias = (rng.standard_normal(s).astype(np.float32) for s in ((k,), (k,), (n,)))
    r = rng.standard_normal((rows, n)).astype(np.float32)
    w16, w216 = ops.to_bf16(w), ops.to_bf16(w2)
    for bf16 in (False, True):
        wv, w2v = ((ops.bf16_to_f32(a) if bf16 else b).astype(np.float64) for a, b in ((w16, w), (w216, w2)))
        wa, w2a = (w16, w216) if bf16 else (w, w2)
        for form in ("plain", "rms", "swiglu", "residual", "ln", "ln+gelu"):
            naive = np.zeros((rows, n))
            for i in range(rows):
                xi = [float(v) for v in x[i]]
                if form in ("rms", "swiglu"):
                    rms = math.sqrt(sum(v * v for v in xi) / k + eps)
                    xi = [v / rms * float(gamma[c]) for c, v in enumerate(xi)]
                if form in ("ln", "ln+gelu"):
                    mu = sum(xi) / k
                    sd = math.sqrt(sum((v - mu) ** 2 for v in xi) / k + eps)
                    xi = [(v - mu) / sd * float(gamma[c]) + float(beta[c]) for c, v in enumerate(xi)]
                for j in range(n):
                    a = sum(xi[c] * wv[j, c] for c in range(k)) + float(bias[j])
                    if form == "swiglu":
                        a = a / (1.0 + math.exp(-a)) * sum(xi[c] * w2v[j, c] for c in range(k))
                    if form == "ln+gelu":
                        a = 0.5 * a * (1.0 + math.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a ** 3)))
                    if form == "residual":
                        a += float(r[i, j])
                    naive[i, j] = a
            got = D.gemv64(x, wa, gamma=gamma if form not in ("plain", "residual") else None, beta=beta if form.startswith("ln") else None,
                           eps=eps, layernorm=form.startswith("ln"), gelu_tanh=form == "ln+gelu", w2=w2a if form == "swiglu" else None,
                           swiglu=form == "swiglu", bias=bias, r=r if form == "residual" else None, bf16=bf16)
            assert np.abs(got - naive).max() < 1e-13, (form, bf16)
    q, kk, v = D.segments(np.arange(12.0).reshape(2, 6), 2, 2)
    assert q.tolist() == [[0, 1], [6, 7]] and kk.tolist() == [[2, 3], [8, 9]] and v.tolist() == [[4, 5], [10, 11]]
    assert np.abs(D.dot64(x.astype(np.float64), w, block=2) - x.astype(np.float64) @ w.astype(np.float64).T).max() < 1e-13


def test_qkv_rope64_against_naive_loops():
    rng = np.random.default_rng(12)
    heads, kv, d, k, positions, pos, eps = 3, 1, 6, 8, 4, 2, 1e-6
    n = (heads + 2 * kv) * d
    x, w, gamma, bias = (rng.standard_normal(s).astype(np.float32) for s in ((k,), (n, k), (k,), (n,)))
    ang = rng.standard_normal((positions, d // 2))
    cos_t, sin_t = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    rms = math.sqrt(sum(float(v) ** 2 for v in x) / k + eps)
    xn = [float(v) / rms * float(gamma[c]) for c, v in enumerate(x)]
    y = [sum(xn[c] * float(w[j, c]) for c in range(k)) + float(bias[j]) for j in range(n)]

    def rot(vec, nh):
        out = list(vec)
        for h in range(nh):
            for i in range(d // 2):
                a, b = vec[h * d + i], vec[h * d + i + d // 2]
                c, s = float(cos_t[pos, i]), float(sin_t[pos, i])
                out[h * d + i], out[h * d + i + d // 2] = a * c - b * s, a * s + b * c
        return out

    q, kr, vr = D.qkv_rope64(x, gamma, eps, w, bias, heads, kv, d, cos_t, sin_t, pos)
    assert np.abs(q - rot(y[:heads * d], heads)).max() < 1e-13
    assert np.abs(kr - rot(y[heads * d:(heads + kv) * d], kv)).max() < 1e-13
    assert np.abs(vr - y[(heads + kv) * d:]).max() < 1e-13
    t = ops.to_bf16(rng.standard_normal((3, k)).astype(np.float32))
    assert np.array_equal(D.embed_row(t, 2, bf16=True), ops.bf16_to_f32(t[2])) and not D.embed_row(t, 3, bf16=True).any()
    assert np.array_equal(D.widen(t, True), ops.bf16_to_f32(t).astype(np.float64))
