"""The fused-projection entry points without a GPU: the four symbols are declared, exported and bound with their arity, answer NULL
as declared and refuse, before the device is touched and with the outputs as they were, rows that do not fit the outputs and
positions past the RoPE table.  Also tests/quant_proj_ref64.py against itself and against tests/llm_ref64.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import fp8_fixture as F8
from tests import gguf_fixture as GG
from tests import llm_ref64 as R64
from tests import quant_proj_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
F32, F64 = np.float32, np.float64

SYMBOLS = {"kjarni_hip_op_fused_proj_fp8": 23, "kjarni_hip_op_fused_proj_ggml": 31, "kjarni_hip_op_qembed": 8, "kjarni_hip_op_q8k_quantize": 8}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    for name, arity in SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/kjarni_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is C.c_int32
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name


def test_null_pointers_are_refused_before_the_device():
    f = (C.c_float * 1024)()
    p3 = (C.c_void_p * 3)(C.addressof(f), C.addressof(f), C.addressof(f))
    i3 = (C.c_int32 * 3)(1, 1, 1)
    l3 = (C.c_int64 * 3)(8, 8, 8)
    args = [0, 0, p3, p3, i3, i3, i3, 16, f, 1, 16, 1, None, 0.0, None, None, 0, 0, p3, i3, l3, 0, 0]
    for at in (2, 3, 4, 5, 6, 8, 18, 19, 20):      # codes, scales, scale_rows, scale_cols, n, x, y, out_rows, ldy
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_fused_proj_fp8(*bad) == E.NULL_POINTER, at
    args = [0, 0, p3, i3, i3, 256, f, 1, 256, 1, None, 0.0, None, 0, None, None, 0, 0, p3, i3, l3, 0, 0, 0, None, None, 0, 0, None, None, None]
    for at in (2, 3, 4, 6, 18, 19, 20):            # blocks, types, n, x, y, out_rows, ldy
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_fused_proj_ggml(*bad) == E.NULL_POINTER, at
    u = (C.c_uint32 * 4)()
    args = [0, u, 4, C.cast(f, C.c_void_p), 8, 1, 256, f]
    for at in (1, 3, 7):
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_qembed(*bad) == E.NULL_POINTER, at
    args = [0, f, 1, 256, 256, C.cast(f, C.c_void_p), f, f]
    for at in (1, 5, 6, 7):
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_q8k_quantize(*bad) == E.NULL_POINTER, at
    assert not any(f)


# ---- the entries' own checks: INVALID_CONFIG before any GPU work ---------------------------------------------------------------

def _refused(call, ys):
    with pytest.raises(KjarniException) as e:
        call()
    assert e.value.code == E.INVALID_CONFIG, str(e.value)
    assert all((y == 7.0).all() for y in ys), "a refused call wrote its output"


def test_entries_refuse_rows_outside_the_outputs_and_positions_past_the_table():
    k = 256
    x = np.zeros((3, k), F32)
    sevens = lambda *shape: np.full(shape, 7.0, F32)  # noqa: E731
    f8 = [(np.zeros((n, k), np.uint8), np.ones((1, 1), F32)) for n in (16, 8, 8)]
    for kw in (dict(row_off=11), dict(row_off=11, offset_on_device=True), dict(row_off=-1), dict(rows=4)):
        ys = [sevens(3, 16), sevens(12, 8), sevens(12, 8)]
        _refused(lambda: ops.fused_proj_fp8(1, f8, x, kw.pop("rows", 2), ys, in_place=True, **kw), ys)
    ys = [sevens(1, 16)]
    _refused(lambda: ops.fused_proj_fp8(0, f8[:1], x, 2, ys, in_place=True), ys)                         # y[0] has one row
    ys = [sevens(2, 15)]
    _refused(lambda: ops.fused_proj_fp8(0, f8[:1], x, 2, ys, in_place=True), ys)                         # ldy < n
    ys = [sevens(2, 16)]
    _refused(lambda: ops.fused_proj_fp8(0, f8[:1], np.zeros((3, k + 2), F32), 2, ys, in_place=True), ys)  # ldx % 4
    _refused(lambda: ops.fused_proj_fp8(2, [f8[0], f8[1]], x, 2, ys, gamma=np.ones(k, F32), in_place=True), ys)   # gate / up of different n
    _refused(lambda: ops.fused_proj_fp8(0, [(f8[0][0], np.ones((3, 1), F32))], x, 2, ys, in_place=True), ys)      # a scale shape of no kind
    rng = np.random.default_rng(0)
    gg = [(8, GG.random_blocks(8, n, k, rng)) for n in (16, 8, 8)]
    tab = np.ones((12, 4), F32)
    for kw in (dict(row_off=11), dict(row_off=11, offset_on_device=True), dict(row_off=9, positions=10),
               dict(row_off=9, positions=10, offset_on_device=True), dict(head_dim=6), dict(bias=np.ones(32, F32), bias_off=(0, 16, 25))):
        ys = [sevens(3, 16), sevens(12, 8), sevens(12, 8)]
        t = tab[:kw.pop("positions", 12)]
        hd = kw.pop("head_dim", 8)
        _refused(lambda: ops.fused_proj_ggml(1, gg, x, 2, ys, head_dim=hd, cos=t[:, :hd // 2], sin=t[:, :hd // 2], in_place=True, **kw), ys)
    ys = [sevens(3, 16)]
    _refused(lambda: ops.fused_proj_ggml(2, gg[:2], x, 2, ys, in_place=True), ys)                        # gate / up of different n
    _refused(lambda: ops.fused_proj_ggml(0, [(2, gg[0][1])], x, 2, ys, in_place=True), ys)               # Q4_0: not a matrix type here
    with pytest.raises(KjarniException) as e:
        ops.qembed([0], 8, gg[0][1][:, :136], 16, 128)                                                    # k % 256
    assert e.value.code == E.INVALID_CONFIG
    with pytest.raises(KjarniException) as e:
        ops.q8k_quantize(np.zeros((1, 250), F32), 256)
    assert e.value.code == E.INVALID_CONFIG
    # the wrappers hold the arrays they pass against the sizes the entry reads
    ys = [sevens(2, 16)]
    for call in (lambda: ops.fused_proj_fp8(0, f8[:1], x, 2, ys, gamma=np.ones(k - 1, F32)),
                 lambda: ops.fused_proj_fp8(0, f8[:1], x, 2, ys, bias=np.ones(15, F32)),
                 lambda: ops.fused_proj_fp8(1, f8, x, 2, [ys[0], sevens(12, 8), sevens(12, 8)], bias=np.ones(16, F32)),
                 lambda: ops.fused_proj_fp8(0, f8[:1], x, 2, ys, r=np.ones((1, 16), F32)),
                 lambda: ops.fused_proj_fp8(1, [f8[0], f8[1], (f8[2][0][:, :128], f8[2][1])], x, 2, [ys[0], sevens(12, 8), sevens(12, 8)]),
                 lambda: ops.fused_proj_ggml(0, gg[:1], x, 2, ys, gamma=np.ones(k + 1, F32)),
                 lambda: ops.fused_proj_ggml(0, [(8, gg[0][1][:, :-34])], x, 2, ys),
                 lambda: ops.fused_proj_ggml(0, gg[:1], x, 2, ys, r=np.ones((1, 16), F32)),
                 lambda: ops.qembed([0], 8, gg[0][1], 17, 256)):
        with pytest.raises(ValueError):
            call()


# ---- the reference against itself ---------------------------------------------------------------------------------------------

def test_reference_rope_is_llm_ref64s_rotation():
    cfg = GG.LLAMA_Q
    ref = R64.Ref64({}, cfg)
    heads, d = cfg["num_attention_heads"], ref.d
    rng = np.random.default_rng(1)
    y = rng.standard_normal((5, heads * d))
    off = 7
    want = ref.rope(y.reshape(5, heads, d), off + np.arange(5)).reshape(5, -1)
    got = R.rope64(y, d, ref.cos[:, :d // 2], ref.sin[:, :d // 2], off)
    assert np.array_equal(got, want)
    out = R.finish64("qkv", [y, y[:, :2 * d], y[:, :d]], None, None, dict(head_dim=d, cos=ref.cos[:, :d // 2], sin=ref.sin[:, :d // 2], off=off))
    assert np.array_equal(out[0], want) and np.array_equal(out[1], want[:, :2 * d]) and np.array_equal(out[2], y[:, :d])   # V is not rotated


def test_q6k_integer_form_equals_the_dequantized_form_on_exact_codes():
    rng = np.random.default_rng(2)
    n, k, m = 5, 768, 3
    blocks = GG.random_blocks(14, n, k, rng)
    xq = rng.integers(-127, 128, (m, k))
    xd = rng.uniform(0.5, 2.0, (m, k // 256)).astype(F32)
    x = xq.astype(F64) * np.repeat(xd.astype(F64), 256, axis=1)                 # activations that their codes represent exactly
    codes, sc, d = GG.q6k_codes(blocks.reshape(-1))
    w = (d.astype(F64)[:, None] * (codes - 32) * np.repeat(sc.astype(F64), 16, axis=1)).reshape(n, k)   # dequantized in float64
    a, b = R.q6k_on_codes64(xq, xd, blocks, n, k), x @ w.T
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert np.array_equal(R.ggml_product64(x, 14, blocks, n, k, (xq, xd)), a)
    # on codes of its own making the integer form is gguf_fixture.linear_reference
    xf = rng.standard_normal((m, k)).astype(F32)
    q, s = GG.q8k_quantize(xf)
    assert np.array_equal(R.q6k_on_codes64(q, s, blocks, n, k), GG.linear_reference(xf, 14, blocks, n, k))


def test_one_hot_rows_read_single_weights_on_the_cpu():
    rng = np.random.default_rng(3)
    n, k = 6, 512
    pos = [0, 31, 32, 255, 256, k - 1]
    x = np.zeros((len(pos), k), F32)
    x[np.arange(len(pos)), pos] = 1.0
    for t in (8, 12, 14):
        blocks = GG.random_blocks(t, n, k, rng)
        w = GG.dequantize(t, blocks, n, k)
        y = R.ggml_product64(x, t, blocks, n, k)
        assert np.array_equal(y, w[:, pos].T.astype(F64)) and np.array_equal(y.astype(F32), w[:, pos].T)
    for kind in F8.KINDS:
        codes, scale = F8.quantize(rng.standard_normal((n, k)).astype(F32) * 0.05, kind, rng)
        w = F8.dequantize(codes, scale, kind)
        assert np.array_equal(x.astype(F64) @ R.fp8_weights64(codes, scale, kind).T, w[:, pos].T.astype(F64))


def test_reference_steps():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3, 64))
    g = rng.standard_normal(64)
    assert np.allclose(R.rms_norm64(x, g, 1e-5), x / np.sqrt((x * x).mean(-1, keepdims=True) + 1e-5) * g, rtol=0, atol=1e-15)
    a, b = rng.standard_normal((3, 4)), rng.standard_normal((3, 4))
    bias, r = rng.standard_normal(4), rng.standard_normal((3, 4))
    (y,) = R.finish64("swiglu", [a, b], [bias])
    assert np.allclose(y, (a + bias) / (1 + np.exp(-(a + bias))) * b, rtol=0, atol=1e-15)
    (y,) = R.finish64("plain", [a], [bias], r)
    assert np.array_equal(y, a + bias + r)
    assert R.silu64(np.array([-90.0]))[0] < 0 and np.isfinite(R.silu64(np.array([-90.0, 90.0]))).all()
    q, d, deq = R.q8k_f32(np.array([[0.5, -0.5, 2.5, -2.5, 126.5, -126.5, 127.0] + [0.0] * 249], F32))
    assert q[0, :7].tolist() == [1, -1, 3, -3, 127, -127, 127] and d[0, 0] == 1.0 and np.array_equal(deq[0, :7], q[0, :7].astype(F32))
