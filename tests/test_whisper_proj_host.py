"""The Whisper projection and front-end entry points without a GPU: kjarni_hip_op_gemv_rows, kjarni_hip_gemv_rows_route and the six
front-end hooks are declared, exported and bound with their arity, answer NULL as declared, and refuse what their checks and the
launcher's rule refuse -- INVALID_CONFIG before any GPU work, with every output still holding its sentinel.  Also the route rule
restated in Python (tests/whisper_proj_ref64.py) against a table worked out by hand and against gemv_rows_route itself over a grid
of arguments, and the float64 reference against hand-computed cases and oracle/whisper_oracle.py's log-mel pieces."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from oracle import whisper_oracle as WO
from tests import whisper_proj_ref64 as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
F32 = np.float32

SYMBOLS = {"kjarni_hip_op_gemv_rows": 35, "kjarni_hip_gemv_rows_route": 14, "kjarni_hip_op_mel_frames": 9, "kjarni_hip_op_mel_power": 8,
           "kjarni_hip_op_mel_log_normalize": 7, "kjarni_hip_op_im2col3": 10, "kjarni_hip_op_add_rows": 8, "kjarni_hip_op_decoder_embed": 13}
SENTINEL = 7.0
PASSES = (E.OK, E.GPU_UNAVAILABLE)   # past the check: only the device may be missing
BIAS, GELU, RES = W.EPI_BIAS, W.EPI_BIAS_GELU, W.EPI_BIAS_RESIDUAL


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


def test_the_binding_names_the_routes_as_the_reference_does():
    assert (ops.GEMV_ROWS_NOTHING, ops.GEMV_ROWS_ONE_FAST, ops.GEMV_ROWS_ONE_FAST_EMBED, ops.GEMV_ROWS_STAGED_FAST, ops.GEMV_ROWS_HEAD,
            ops.GEMV_ROWS_STAGED, ops.GEMV_ROWS_GENERAL, ops.GEMV_ROWS_GEMM, ops.GEMV_ROWS_REFUSED) == \
        (W.NOTHING, W.ONE_FAST, W.ONE_FAST_EMBED, W.STAGED_FAST, W.HEAD, W.STAGED, W.GENERAL, W.GEMM, W.REFUSED)
    assert (ops.EPI_BIAS, ops.EPI_BIAS_GELU, ops.EPI_BIAS_RESIDUAL) == (BIAS, GELU, RES)
    assert (ops.MISALIGN_X, ops.MISALIGN_W, ops.MISALIGN_GAMMA, ops.MISALIGN_BETA) == (W.MIS_X, W.MIS_W, W.MIS_GAMMA, W.MIS_BETA)


def _p(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


# ---- kjarni_hip_op_gemv_rows ----------------------------------------------------------------------------------------------------------

def _gemv(rows=2, k=16, n_out=6, x_rows=None, ldx=None, gamma=False, beta=None, residual=False, ldr=None, r_is_y0=0, seg=0, ldy0=None,
          ldy12=None, out_rows=(4, 6, 6), row_off=0, on_device=0, epi=BIAS, embed=False, word=True, vocab=3, max_pos=3, pos=0, pos_dev=0,
          loose_embed=False, raw=False, norm=False, misalign=0, null_y=None, x=True):
    """A call with valid zero buffers for the sizes given; every output starts as a sentinel that a refused call must leave alone.
    Returns the error code."""
    kk, nn = max(k, 1), max(n_out, 1)
    ldx = k if ldx is None else ldx
    beta = gamma if beta is None else beta
    cols0 = seg if seg > 0 else nn
    ldy0 = cols0 if ldy0 is None else ldy0
    ldy12 = seg if ldy12 is None else ldy12
    ldr = nn if ldr is None else ldr
    xa = np.ones((max(rows, 1) if x_rows is None else max(x_rows, 1), max(ldx, kk)), F32) if x and not embed else None
    w = np.zeros((nn, kk), F32)
    ys = [np.full((max(out_rows[i], 1), max(ld, c, 1)), SENTINEL, F32) for i, (ld, c) in enumerate(((ldy0, cols0), (ldy12, seg), (ldy12, seg)))]
    yp = (C.c_void_p * 3)(*[None if null_y == i else y.ctypes.data for i, y in enumerate(ys)])
    orows = (C.c_int32 * 3)(*out_rows)
    vec = np.ones(kk, F32)
    r = np.zeros((max(rows, 1), max(ldr, nn)), F32) if residual else None
    ida = np.array([1], np.uint32) if embed else None
    wt = np.zeros((max(vocab, 1), kk), F32) if (embed or loose_embed) and word else None
    pt = np.zeros((max(max_pos, 1), kk), F32) if embed and max_pos > 0 else None
    ro, no = (np.full(kk, SENTINEL, F32) if f else None for f in (raw, norm))
    route = C.c_int32(-5)
    rc = L.kjarni_hip_op_gemv_rows(0, _p(xa), max(rows, 1) if x_rows is None else x_rows, ldx, rows, _p(vec) if gamma else None,
                                   _p(vec) if beta else None, 1e-5, _p(w), None, _p(r), ldr, r_is_y0, n_out, k, seg, yp, orows, ldy0, ldy12,
                                   row_off, on_device, epi, None if ida is None else ida.ctypes.data_as(_ffi._u32p), _p(wt), vocab, _p(pt), max_pos,
                                   pos, pos_dev, 1.0, _p(ro), _p(no), misalign, C.byref(route))
    if rc != E.OK:
        assert all((y == SENTINEL).all() for y in ys) and all(t is None or (t == SENTINEL).all() for t in (ro, no)), "a refused call wrote its output"
        assert route.value == -5, "a refused call wrote its route"
    return rc


SEG = dict(seg=2, n_out=6)
ONE = dict(rows=1, k=512)
EMB = dict(rows=1, k=512, embed=True, gamma=True)


@pytest.mark.parametrize("kw", [
    # the hook's own checks: sizes, strides, rows that do not fit
    dict(rows=17), dict(rows=-2), dict(rows=3, x_rows=2), dict(x_rows=65), dict(k=0), dict(k=-4), dict(k=(1 << 16) + 4),
    dict(n_out=-2), dict(n_out=(1 << 17) + 1), dict(n_out=1 << 13, k=1 << 14), dict(ldx=12), dict(ldx=(1 << 18) + 4),
    dict(ldy0=5), dict(ldy0=0), dict(residual=True, epi=RES, ldr=5), dict(out_rows=(1, 6, 6)), dict(out_rows=(0, 6, 6)),
    dict(out_rows=(4097, 6, 6)), dict(null_y=0), dict(epi=-1), dict(epi=7), dict(misalign=16), dict(misalign=-1),
    dict(residual=True, r_is_y0=1, epi=RES), dict(seg=-1), dict(row_off=-1, **SEG), dict(row_off=5, **SEG), dict(row_off=5, on_device=1, **SEG),
    dict(row_off=4, out_rows=(4, 6, 5), **SEG), dict(row_off=4, out_rows=(4, 5, 6), **SEG), dict(ldy12=1, **SEG), dict(ldy0=1, **SEG),
    dict(null_y=1, **SEG), dict(null_y=2, **SEG), dict(r_is_y0=1, epi=RES, **SEG), dict(out_rows=(4, 0, 6), **SEG),
    dict(vocab=-1, **EMB), dict(vocab=(1 << 17) + 1, **EMB), dict(max_pos=-1, **EMB), dict(max_pos=(1 << 16) + 1, **EMB), dict(pos=-1, **EMB),
    dict(loose_embed=True), dict(pos_dev=1),
    # the launcher's rule, asked before any GPU work
    dict(gamma=True, beta=False), dict(gamma=True, beta=False, **ONE),                                          # LayerNorm without beta
    dict(epi=RES), dict(epi=RES, **ONE),                                                                        # a residual epilogue without one
    dict(epi=GELU), dict(epi=GELU, **ONE), dict(epi=RES, residual=True, gamma=True), dict(epi=RES, r_is_y0=1, gamma=True, **ONE),
    dict(epi=2), dict(epi=3), dict(epi=4), dict(epi=6, residual=True), dict(epi=2, gamma=True), dict(epi=6, rows=9, residual=True),
    dict(epi=GELU, rows=9), dict(epi=2, k=18, ldx=18),                                                          # the pairs hold on the GEMM route too
    dict(seg=1, n_out=6), dict(seg=1, n_out=4, **ONE),                                                          # n_out above 3 seg
    dict(rows=9, gamma=True), dict(rows=9, **SEG), dict(k=18, ldx=18, gamma=True), dict(k=18, ldx=18, seg=2), dict(ldx=18, gamma=True),
    dict(misalign=1, gamma=True), dict(misalign=2, **SEG), dict(misalign=3, gamma=True, **SEG),                 # gamma or segments on the GEMM route
    dict(raw=True), dict(norm=True, gamma=True), dict(norm=True, gamma=True, rows=2, k=512), dict(norm=True, gamma=True, rows=1, k=768),
    dict(norm=True, gamma=True, rows=1, k=1024), dict(norm=True, gamma=True, misalign=1, **ONE), dict(norm=True, gamma=True, misalign=2, **ONE),
    dict(norm=True, gamma=True, misalign=4, **ONE), dict(norm=True, gamma=True, misalign=8, **ONE), dict(norm=True, gamma=True, ldx=514, **ONE),
    dict(norm=True, **ONE), dict(raw=True, **ONE), dict(raw=True, gamma=True, **ONE), dict(raw=True, rows=1, k=2048),   # no kernel would write them
    dict(rows=1, k=512, embed=True), dict(rows=1, k=512, embed=True, gamma=True, epi=GELU), dict(rows=1, k=2048, embed=True, gamma=True),
    dict(rows=2, k=512, embed=True, gamma=True), dict(rows=1, k=768, embed=True, gamma=True), dict(word=False, **EMB),
    dict(misalign=4, **EMB), dict(misalign=8, **EMB), dict(misalign=2, **EMB), dict(epi=RES, residual=True, rows=1, k=512, embed=True),
], ids=str)
def test_gemv_rows_refuses(kw):
    assert _gemv(**kw) == E.INVALID_CONFIG, kw


def test_gemv_rows_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(rows=0), dict(rows=-1), dict(n_out=0), dict(n_out=-1), dict(rows=8, out_rows=(8, 6, 6)), dict(rows=16, out_rows=(16, 6, 6)),
               dict(rows=1, x_rows=64), dict(k=1), dict(k=18, ldx=19), dict(ldx=20), dict(ldy0=9), dict(gamma=True), dict(gamma=True, epi=GELU),
               dict(residual=True, epi=RES), dict(residual=True, epi=RES, ldr=9), dict(r_is_y0=1, epi=RES), dict(r_is_y0=1, epi=RES, rows=9, out_rows=(9, 6, 6)),
               dict(**SEG), dict(row_off=4, **SEG), dict(row_off=4, on_device=1, **SEG), dict(ldy12=5, ldy0=3, **SEG), dict(gamma=True, **SEG),
               dict(seg=2, n_out=5), dict(seg=3, n_out=6), dict(**ONE), dict(norm=True, gamma=True, **ONE),
               dict(norm=True, gamma=True, rows=1, k=2048), dict(norm=True, raw=True, **EMB), dict(**EMB), dict(raw=True, **EMB), dict(vocab=0, **EMB), dict(max_pos=0, **EMB), dict(pos=9, **EMB),
               dict(pos=2, pos_dev=1, **EMB), dict(seg=4, n_out=12, **EMB), dict(misalign=1), dict(misalign=2), dict(misalign=4, gamma=True),
               dict(misalign=12, gamma=True, **ONE), dict(misalign=8, **ONE), dict(n_out=1 << 17, k=512, rows=1), dict(out_rows=(4096, 6, 6))):
        assert _gemv(**kw) in PASSES, kw
    assert _gemv() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


def test_gemv_rows_null_pointers():
    f = (C.c_float * 256)()
    yp, orows, route = (C.c_void_p * 3)(C.addressof(f), None, None), (C.c_int32 * 3)(4, 0, 0), C.c_int32(-5)
    args = [0, f, 2, 16, 2, None, None, 0.0, f, None, None, 0, 0, 6, 16, 0, yp, orows, 6, 0, 0, 0, 0, None, None, 0, None, 0, 0, 0, 1.0, None, None, 0,
            C.byref(route)]
    for at in (1, 8, 16, 17, 34):                                          # x (without embed_id), w, y, out_rows, route_out
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_gemv_rows(*bad) == E.NULL_POINTER
    assert route.value == -5 and not any(f)
    assert L.kjarni_hip_gemv_rows_route(1, 1, 512, 512, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == E.NULL_POINTER


# ---- the front-end hooks --------------------------------------------------------------------------------------------------------------

def _front(name, **kw):
    """One call of a front-end hook with valid sentinel buffers for the sizes given.  Returns the error code; a refusal must leave
    the outputs alone."""
    S = lambda *shape: np.full([max(int(s), 1) for s in shape], SENTINEL, F32)  # noqa: E731
    if name == "mel_frames":
        a = dict(n=10, n_fft=8, hop=4, n_frames=3, ld=8)
        a.update(kw)
        outs = [S(a["n_frames"], a["ld"])]
        rc = L.kjarni_hip_op_mel_frames(0, _p(S(a["n"])), a["n"], _p(S(a["n_fft"])), a["n_fft"], a["hop"], a["n_frames"], a["ld"], _p(outs[0]))
    elif name == "mel_power":
        a = dict(ld_dft=16, im_off=8, n_bins=5, ld_out=8, n_frames=2)
        a.update(kw)
        outs = [S(a["n_frames"], a["ld_out"])]
        rc = L.kjarni_hip_op_mel_power(0, _p(S(a["n_frames"], a["ld_dft"])), a["ld_dft"], a["im_off"], a["n_bins"], a["ld_out"], a["n_frames"], _p(outs[0]))
    elif name == "mel_log_normalize":
        a = dict(ld=8, n_mels=5, n_frames=2, ld_out=6)
        a.update(kw)
        outs = [S(a["n_frames"], a["ld"]), S(a["n_frames"], a["ld_out"])]
        rc = L.kjarni_hip_op_mel_log_normalize(0, _p(outs[0]), a["ld"], a["n_mels"], a["n_frames"], a["ld_out"], _p(outs[1]))
    elif name == "im2col3":
        a = dict(ldx=4, t_in=5, channels=3, stride=1, pad=1, t_out=5, ld_cols=12)
        a.update(kw)
        outs = [S(a["t_out"], a["ld_cols"])]
        rc = L.kjarni_hip_op_im2col3(0, _p(S(a["t_in"], a["ldx"])), a["ldx"], a["t_in"], a["channels"], a["stride"], a["pad"], a["t_out"], a["ld_cols"],
                                     _p(outs[0]))
    elif name == "add_rows":
        a = dict(rows=7, hidden=5, period=3, table_rows=2, alloc=3)
        a.update(kw)
        outs = [S(a["rows"], a["hidden"])]
        rc = L.kjarni_hip_op_add_rows(0, _p(outs[0]), a["rows"], a["hidden"], a["period"], _p(S(a["alloc"], a["hidden"])), a["table_rows"], a["alloc"])
    else:
        a = dict(n=2, hidden=5, vocab=4, max_pos=6, offset=1, on_device=0, pos=True)
        a.update(kw)
        outs = [S(a["n"], a["hidden"])]
        ids = np.zeros(max(a["n"], 1), np.uint32)
        rc = L.kjarni_hip_op_decoder_embed(0, ids.ctypes.data_as(_ffi._u32p), a["n"], a["hidden"], a["vocab"], _p(S(a["vocab"], a["hidden"])),
                                           _p(S(a["max_pos"], a["hidden"])) if a["pos"] else None, a["max_pos"], a["offset"], a["on_device"], 0, 0,
                                           _p(outs[0]))
    if rc != E.OK:
        assert all((o == SENTINEL).all() for o in outs), "a refused call wrote its output"
    return rc


@pytest.mark.parametrize("name,kw", [
    ("mel_frames", dict(n=0)), ("mel_frames", dict(n_fft=1)), ("mel_frames", dict(n_fft=4097, ld=4100)), ("mel_frames", dict(hop=0)),
    ("mel_frames", dict(n_frames=0)), ("mel_frames", dict(ld=7)), ("mel_frames", dict(ld=8193)), ("mel_frames", dict(n_frames=(1 << 16) + 1)),
    ("mel_power", dict(n_frames=0)), ("mel_power", dict(n_bins=-1)), ("mel_power", dict(n_bins=9)), ("mel_power", dict(im_off=-1)),
    ("mel_power", dict(im_off=12)), ("mel_power", dict(ld_out=0, n_bins=0)), ("mel_power", dict(ld_dft=8193, im_off=0)),
    ("mel_log_normalize", dict(n_frames=0)), ("mel_log_normalize", dict(n_mels=0)), ("mel_log_normalize", dict(ld=4)),
    ("mel_log_normalize", dict(ld_out=4)), ("mel_log_normalize", dict(ld=4097)),
    ("im2col3", dict(t_in=0)), ("im2col3", dict(channels=0)), ("im2col3", dict(ldx=2)), ("im2col3", dict(stride=0)), ("im2col3", dict(pad=-1)),
    ("im2col3", dict(t_out=0)), ("im2col3", dict(ld_cols=8)), ("im2col3", dict(stride=17)),
    ("add_rows", dict(rows=0)), ("add_rows", dict(hidden=0)), ("add_rows", dict(period=0)), ("add_rows", dict(table_rows=-1)),
    ("add_rows", dict(table_rows=4, alloc=3)), ("add_rows", dict(alloc=0, table_rows=0)),
    ("decoder_embed", dict(n=0)), ("decoder_embed", dict(n=65)), ("decoder_embed", dict(hidden=0)), ("decoder_embed", dict(vocab=0)),
    ("decoder_embed", dict(max_pos=-1)), ("decoder_embed", dict(offset=-1)), ("decoder_embed", dict(offset=-1, on_device=1)),
    ("decoder_embed", dict(max_pos=0)),
], ids=str)
def test_front_end_refuses(name, kw):
    assert _front(name, **kw) == E.INVALID_CONFIG, (name, kw)


def test_front_end_accepts_the_edges_of_its_checks():
    for name, kw in (("mel_frames", {}), ("mel_frames", dict(n=1)), ("mel_frames", dict(ld=9)), ("mel_frames", dict(n_frames=40)),
                     ("mel_power", {}), ("mel_power", dict(n_bins=0)), ("mel_power", dict(n_bins=8)), ("mel_power", dict(im_off=11)),
                     ("mel_log_normalize", {}), ("mel_log_normalize", dict(n_mels=6)), ("mel_log_normalize", dict(n_frames=1)),
                     ("im2col3", {}), ("im2col3", dict(ld_cols=9)), ("im2col3", dict(pad=0)), ("im2col3", dict(stride=2, t_out=9)),
                     ("add_rows", {}), ("add_rows", dict(table_rows=0)), ("add_rows", dict(table_rows=3)), ("add_rows", dict(period=100)),
                     ("decoder_embed", {}), ("decoder_embed", dict(offset=6)), ("decoder_embed", dict(offset=9, on_device=1)),
                     ("decoder_embed", dict(pos=False, max_pos=0)), ("decoder_embed", dict(n=64))):
        assert _front(name, **kw) in PASSES, (name, kw)


def test_front_end_null_pointers():
    f = (C.c_float * 64)()
    u = (C.c_uint32 * 4)()
    assert L.kjarni_hip_op_mel_frames(0, None, 10, f, 8, 4, 3, 8, f) == L.kjarni_hip_op_mel_frames(0, f, 10, None, 8, 4, 3, 8, f) == \
        L.kjarni_hip_op_mel_frames(0, f, 10, f, 8, 4, 3, 8, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_mel_power(0, None, 16, 8, 5, 8, 2, f) == L.kjarni_hip_op_mel_power(0, f, 16, 8, 5, 8, 2, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_mel_log_normalize(0, None, 8, 5, 2, 6, f) == L.kjarni_hip_op_mel_log_normalize(0, f, 8, 5, 2, 6, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_im2col3(0, None, 4, 5, 3, 1, 1, 5, 12, f) == L.kjarni_hip_op_im2col3(0, f, 4, 5, 3, 1, 1, 5, 12, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_add_rows(0, None, 7, 5, 3, f, 2, 3) == L.kjarni_hip_op_add_rows(0, f, 7, 5, 3, None, 2, 3) == E.NULL_POINTER
    assert L.kjarni_hip_op_decoder_embed(0, None, 2, 5, 4, f, f, 6, 1, 0, 0, 0, f) == L.kjarni_hip_op_decoder_embed(0, u, 2, 5, 4, None, f, 6, 1, 0, 0, 0, f) == \
        L.kjarni_hip_op_decoder_embed(0, u, 2, 5, 4, f, f, 6, 1, 0, 0, 0, None) == E.NULL_POINTER
    assert not any(f)


def test_wrappers_check_their_shapes():
    x, w, y = np.zeros((2, 16), F32), np.zeros((6, 16), F32), np.zeros((2, 6), F32)
    with pytest.raises(ValueError):
        ops.gemv_rows(x, w, 2, [y, y])
    with pytest.raises(ValueError):
        ops.gemv_rows(x, w, 2, [y], gamma=np.zeros(8, F32))
    with pytest.raises(ValueError):
        ops.gemv_rows(None, w, 1, [y])
    with pytest.raises(ValueError):
        ops.gemv_rows(x, w, 2, [y], x_raw_out=np.zeros(8, F32))
    with pytest.raises(ValueError):
        ops.decoder_embed([0, 1], np.zeros((4, 5), F32), np.zeros((3, 6), F32), 0, np.zeros((2, 5), F32))
    with pytest.raises(ValueError):
        ops.add_rows(np.zeros((3, 5), F32), 3, np.zeros((3, 4), F32), 3)


# ---- the route rule: a table worked out by hand from launch_gemv_rows, then the rule itself over a grid -------------------------------

LN = dict(gamma=True)
ROUTE_TABLE = [
    (dict(rows=0, n_out=4, k=512), W.NOTHING), (dict(rows=1, n_out=0, k=512), W.NOTHING), (dict(rows=-1, n_out=4, k=512, epi=3), W.NOTHING),
    (dict(rows=1, n_out=1, k=512), W.ONE_FAST), (dict(rows=1, n_out=7, k=2048, **LN), W.ONE_FAST), (dict(rows=1, n_out=5, k=512, epi=GELU, **LN), W.ONE_FAST),
    (dict(rows=1, n_out=5, k=2048, epi=RES), W.ONE_FAST), (dict(rows=1, n_out=12, k=512, seg=4, **LN), W.ONE_FAST),
    (dict(rows=1, n_out=5, k=512, x_raw_out=True), W.REFUSED), (dict(rows=1, n_out=5, k=2048, x_norm_out=True, **LN), W.ONE_FAST),
    (dict(rows=1, n_out=5, k=512, x_raw_out=True, **LN), W.REFUSED), (dict(rows=1, n_out=5, k=512, x_norm_out=True, embed=True, **LN), W.ONE_FAST_EMBED),
    (dict(rows=1, n_out=5, k=512, ldx=516), W.ONE_FAST), (dict(rows=1, n_out=8192, k=512), W.ONE_FAST),
    (dict(rows=1, n_out=12, k=512, seg=4, embed=True, **LN), W.ONE_FAST_EMBED), (dict(rows=1, n_out=5, k=512, embed=True, x_raw_out=True, **LN), W.ONE_FAST_EMBED),
    (dict(rows=1, n_out=5, k=2048, embed=True, **LN), W.REFUSED), (dict(rows=1, n_out=5, k=512, embed=True), W.REFUSED),
    (dict(rows=1, n_out=5, k=512, embed=True, epi=GELU, **LN), W.REFUSED), (dict(rows=2, n_out=5, k=512, embed=True, **LN), W.REFUSED),
    (dict(rows=2, n_out=5, k=512), W.STAGED_FAST), (dict(rows=8, n_out=7, k=512, **LN), W.STAGED_FAST), (dict(rows=8, n_out=5, k=2048, epi=RES), W.STAGED_FAST),
    (dict(rows=6, n_out=5, k=2048, epi=GELU, **LN), W.STAGED_FAST), (dict(rows=8, n_out=8191, k=512), W.STAGED_FAST),
    (dict(rows=2, n_out=8192, k=512, **LN), W.STAGED_FAST), (dict(rows=2, n_out=8192, k=2048), W.STAGED_FAST), (dict(rows=2, n_out=8193, k=512, epi=RES), W.STAGED_FAST),
    (dict(rows=2, n_out=3 * 4096, k=512, seg=4096), W.STAGED_FAST),
    (dict(rows=2, n_out=8192, k=512), W.HEAD), (dict(rows=8, n_out=8207, k=512), W.HEAD), (dict(rows=5, n_out=51865, k=512), W.HEAD),
    (dict(rows=2, n_out=5, k=4), W.STAGED), (dict(rows=8, n_out=5, k=384), W.STAGED), (dict(rows=8, n_out=5, k=1280, **LN), W.STAGED),
    (dict(rows=3, n_out=5, k=5120), W.STAGED), (dict(rows=2, n_out=5, k=512, misalign=4, **LN), W.STAGED), (dict(rows=2, n_out=5, k=512, misalign=8, **LN), W.STAGED),
    (dict(rows=8, n_out=5, k=1024), W.STAGED), (dict(rows=8, n_out=5, k=2044), W.STAGED), (dict(rows=2, n_out=8192, k=768), W.STAGED),
    (dict(rows=1, n_out=5, k=384), W.GENERAL), (dict(rows=1, n_out=5, k=1280, epi=GELU, **LN), W.GENERAL), (dict(rows=4, n_out=5, k=5120), W.GENERAL),
    (dict(rows=8, n_out=5, k=5120, epi=RES), W.GENERAL), (dict(rows=1, n_out=5, k=512, misalign=4, **LN), W.GENERAL),
    (dict(rows=1, n_out=5, k=2048, misalign=8, **LN), W.GENERAL), (dict(rows=8, n_out=5, k=2052), W.GENERAL), (dict(rows=1, n_out=5, k=1024), W.GENERAL),
    (dict(rows=9, n_out=5, k=512), W.GEMM), (dict(rows=2, n_out=5, k=510, ldx=512), W.GEMM), (dict(rows=2, n_out=5, k=512, ldx=514), W.GEMM),
    (dict(rows=2, n_out=5, k=512, misalign=1), W.GEMM), (dict(rows=1, n_out=5, k=512, misalign=2, epi=RES), W.GEMM), (dict(rows=16, n_out=5, k=18, ldx=18), W.GEMM),
    (dict(rows=9, n_out=5, k=512, **LN), W.REFUSED), (dict(rows=9, n_out=6, k=512, seg=2), W.REFUSED), (dict(rows=2, n_out=5, k=512, misalign=1, **LN), W.REFUSED),
    (dict(rows=9, n_out=5, k=512, epi=GELU), W.REFUSED), (dict(rows=9, n_out=5, k=512, epi=2), W.REFUSED),
    (dict(rows=1, n_out=5, k=512, epi=GELU), W.REFUSED), (dict(rows=2, n_out=5, k=512, epi=RES, **LN), W.REFUSED), (dict(rows=2, n_out=5, k=384, epi=4), W.REFUSED),
    (dict(rows=2, n_out=5, k=512, gamma=True, beta=False), W.REFUSED), (dict(rows=2, n_out=5, k=512, epi=RES, r=False), W.REFUSED),
    (dict(rows=2, n_out=7, k=512, seg=2), W.REFUSED), (dict(rows=2, n_out=5, k=512, x_raw_out=True), W.REFUSED), (dict(rows=1, n_out=5, k=768, x_raw_out=True), W.REFUSED),
    (dict(rows=1, n_out=5, k=512, x_norm_out=True), W.REFUSED), (dict(rows=1, n_out=5, k=512, x_norm_out=True, misalign=4, **LN), W.REFUSED),
    (dict(rows=1, n_out=5, k=512, x_norm_out=True, misalign=1, **LN), W.REFUSED), (dict(rows=1, n_out=5, k=512, x_norm_out=True, ldx=514, **LN), W.REFUSED),
    (dict(rows=1, n_out=5, k=512, x_raw_out=True, embed=True, misalign=2, **LN), W.REFUSED),
]


def test_the_route_rule_restated_gives_the_table():
    for kw, want in ROUTE_TABLE:
        assert W.route(**kw) == want, kw
    assert {w for _, w in ROUTE_TABLE} == set(range(9))


def test_gemv_rows_route_itself_gives_the_table_and_the_restated_rule_over_a_grid():
    for kw, want in ROUTE_TABLE:
        assert ops.gemv_rows_route(**kw) == want, kw
    n = 0
    for rows, k, n_out, epi, gamma in itertools.product((0, 1, 2, 3, 4, 5, 8, 9), (4, 6, 252, 384, 512, 768, 1024, 2048, 2052, 4096, 5120, 5124, 8192),
                                                        (0, 1, 5, 8191, 8192), (BIAS, GELU, 2, RES), (False, True)):
        for seg, mis, extra in itertools.product((0, 3), (0, 1, 2, 4, 8, 12), ("", "embed", "raw", "norm", "beta", "r")):
            kw = dict(rows=rows, n_out=n_out, k=k, seg=seg, epi=epi, gamma=gamma, misalign=mis, embed=extra == "embed", x_raw_out=extra == "raw",
                      x_norm_out=extra == "norm")
            if extra == "beta":
                kw["beta"] = not gamma
            if extra == "r":
                kw["r"] = epi != RES
            assert ops.gemv_rows_route(**kw) == W.route(**kw), kw
            n += 1
    for rows, k in itertools.product(range(1, 10), range(4, 8200, 4)):    # the LDS budget and the widths, every k
        assert ops.gemv_rows_route(rows, 5, k) == W.route(rows, 5, k), (rows, k)
        assert ops.gemv_rows_route(rows, 5, k, ldx=k + 2) == W.route(rows, 5, k, ldx=k + 2) == W.GEMM
    assert n > 50000
    # the budget: rows * k * 4 <= 64 KiB stages, one float more does not
    assert [W.route(r, 5, 2048) for r in (2, 6, 8)] == [W.STAGED_FAST] * 3 and W.route(4, 5, 4096) == W.STAGED and W.route(4, 5, 4100) == W.GENERAL
    assert W.route(3, 5, 5120) == W.STAGED and W.route(4, 5, 5120) == W.GENERAL and W.route(8, 5, 2052) == W.GENERAL


# ---- the reference against hand-computed cases and the oracle's log-mel pieces --------------------------------------------------------

def test_projection_reference_by_hand():
    x = np.array([[1.0, 3.0], [2.0, 2.0]], F32)
    g, b = np.array([2.0, 1.0], F32), np.array([0.5, -0.5], F32)
    ln = W.layer_norm64(x[:1], g, b, 0.0)      # row 0: mean 2, variance 1 -> (-1, 1); row 1: variance 0 -> beta (0 / sqrt(eps) with eps > 0)
    assert np.allclose(ln[0], [-2.0 + 0.5, 1.0 - 0.5], atol=1e-15)
    assert np.allclose(W.layer_norm64(x, g, b, 3.0)[0], [-1.0 + 0.5, 0.5 - 0.5], atol=1e-15)        # eps inside the root: sqrt(1 + 3) = 2
    assert np.array_equal(W.layer_norm64(x, g, b, 1e-5)[1], b.astype(np.float64))
    w = np.array([[1.0, -1.0], [0.5, 2.0], [0.0, 1.0]], F32)
    bias, r = np.array([1.0, 0.0, -1.0], F32), np.array([[10.0, 20.0, 30.0], [1.0, 2.0, 3.0]], F32)
    assert W.gemv_rows64(x, w, bias=bias).tolist() == [[-1.0, 6.5, 2.0], [1.0, 5.0, 1.0]]
    assert W.gemv_rows64(x, w, bias=bias, epi=RES, r=r).tolist() == [[9.0, 26.5, 32.0], [2.0, 7.0, 4.0]]
    got = W.gemv_rows64(x, w, gamma=g, beta=b, eps=3.0, bias=bias, epi=GELU)[0]               # LN row (-0.5, 0): . w + bias = (0.5, -0.25, -1)
    want = [0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0))) for v in (0.5, -0.25, -1.0)]
    assert np.allclose(got, want, atol=1e-15)
    assert abs(float(W.gelu_erf64(1.0)) - 0.8413447460685429) < 1e-15 and float(W.gelu_erf64(0.0)) == 0.0
    q, kk, v = W.segments(np.arange(12.0).reshape(2, 6), 2)
    assert q.tolist() == [[0, 1], [6, 7]] and kk.tolist() == [[2, 3], [8, 9]] and v.tolist() == [[4, 5], [10, 11]]
    word, pos = np.array([[1.0, 2.0], [3.0, 4.0]], F32), np.array([[0.5, 0.25], [10.0, 20.0]], F32)
    assert W.embed64(word, 1, 2.0, pos, 0).tolist() == [6.5, 8.25] and W.embed64(word, 2, 2.0, pos, 1).tolist() == [10.0, 20.0]
    assert W.embed64(word, 0, 1.0, pos, 2).tolist() == [1.0, 2.0] and W.embed64(word, 5, 1.0, None, 0).tolist() == [0.0, 0.0]
    assert W.embed32(word, 1, 2.0, pos, 0).tolist() == [6.5, 8.25] and W.embed32(word, 1, 2.0, pos, 0).dtype == F32
    assert W.decoder_embed32([1, 2, 0], word, pos, 0, False, False).tolist() == [[3.5, 4.25], [10.0, 20.0], [1.0, 2.0]]
    assert W.decoder_embed32([1, 0], word, pos, 1, False, True).tolist() == [[13.0, 24.0], [11.0, 22.0]]
    assert np.array_equal(W.decoder_embed32([1], word, None, 0, True, False)[0], word[1] * np.sqrt(F32(2.0)))
    assert W.bar([0.5]) == 1e-5 and W.bar([-30.0, 2.0]) == 30.0 * 1e-5


def test_front_end_reference_by_hand_and_against_the_oracle():
    a = np.arange(1.0, 6.0, dtype=F32)                        # 1 2 3 4 5
    assert W.pad_reflect(a, 2).tolist() == [3, 2, 1, 2, 3, 4, 5, 4, 3]
    assert W.pad_reflect(a[:2], 3).tolist() == [2, 2, 2, 1, 2, 1, 1, 1]        # left: a[3], a[2] -> the last; a[1].  right: a[0], then before the start
    assert W.pad_reflect(a[:1], 2).tolist() == [1, 1, 1, 1, 1]
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 199, 200, 201, 800):
        s = rng.standard_normal(n).astype(F32)
        assert np.array_equal(W.pad_reflect(s, 200), WO.pad_reflect(s, 200)), n
    win = np.array([1.0, 2.0, 3.0, 4.0], F32)
    fr = W.mel_frames64(a, win, 2, 5, 6)                    # padded 3 2 1 2 3 4 5 4 3: frames at 0, 2, 4 fit, 6 and 8 do not
    assert fr.tolist() == [[3, 4, 3, 8, 0, 0], [1, 4, 9, 16, 0, 0], [3, 8, 15, 16, 0, 0], [0] * 6, [0] * 6]
    s, hann = rng.standard_normal(800).astype(F32), WO.hann_window(400)
    x = WO.pad_reflect(s, 200)
    idx = np.arange(6)[:, None] * 160 + np.arange(400)[None, :]
    assert np.array_equal(W.mel_frames64(s, hann, 160, 6, 400).astype(F32), (x[idx] * hann[None, :]).astype(F32))
    d = np.array([[3.0, 0.0, 9.0, 4.0, 1.0, 9.0]], F32)
    assert W.mel_power64(d, 3, 2, 3).tolist() == [[25.0, 1.0, 0.0]] and W.mel_power32(d, 3, 2, 3).tolist() == [[25.0, 1.0, 0.0]]
    m = np.array([[100.0, 1e-12, 7.0], [1e-3, 0.0, 7.0]], F32)
    lg, out = W.mel_log_normalize64(m, 2)
    floor = math.log10(float(F32(1e-10)))
    assert np.allclose(lg, [[2.0, floor], [math.log10(float(F32(1e-3))), floor]], atol=1e-15) and abs(floor + 10.0) < 1e-8
    assert np.allclose(out, [[1.5, -0.5], [(math.log10(float(F32(1e-3))) + 4.0) / 4.0, -0.5]], atol=1e-15)      # the clamp at 2 - 8 = -6
    x = np.arange(1.0, 11.0, dtype=F32).reshape(5, 2)        # rows (1 2) (3 4) (5 6) (7 8) (9 10)
    c = W.im2col3_64(x, 2, 2, 1, 3, 7)
    assert c.tolist() == [[0, 0, 1, 2, 3, 4, 0], [3, 4, 5, 6, 7, 8, 0], [7, 8, 9, 10, 0, 0, 0]]
    assert W.im2col3_64(x[:, :1], 1, 1, 0, 3, 3).tolist() == [[1, 3, 5], [3, 5, 7], [5, 7, 9]]
    t = np.array([[10.0], [20.0], [30.0]], F32)
    assert W.add_rows32(np.zeros((5, 1), F32), 3, t, 2).ravel().tolist() == [10, 20, 0, 10, 20]
    assert W.add_rows32(np.ones((4, 1), F32), 4, t, 3).ravel().tolist() == [11, 21, 31, 1]
