"""The affine-32 entry points without a GPU: declared, exported and bound with their arity, NULL answered as declared, every
refusal before the device with the outputs as they were, and repack_ggml of the five types against the layout restated in numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import gguf_fixture as G
from tests import gguf_types_fixture as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
F32 = np.float32
SYMBOLS = {"kjarni_hip_op_affine_proj": 23, "kjarni_hip_op_affine_repack": 7, "kjarni_hip_op_affine_dequant": 8}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    for name, arity in SYMBOLS.items():
        assert name in decl and hasattr(L, name), name
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is C.c_int32
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name


def test_null_pointers_are_refused():
    f = (C.c_float * 1024)()
    p3 = (C.c_void_p * 3)(C.addressof(f), C.addressof(f), C.addressof(f))
    i3, l3 = (C.c_int32 * 3)(1, 1, 1), (C.c_int64 * 3)(8, 8, 8)
    args = [0, 0, p3, i3, i3, 32, f, 1, 32, 1, None, 0.0, None, 0, None, None, 0, 0, p3, i3, l3, 0, 0]
    for at in (2, 3, 4, 6, 18, 19, 20):   # blocks, types, n, x, y, out_rows, ldy
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_affine_proj(*bad) == E.NULL_POINTER, at
    v = C.cast(f, C.c_void_p)
    for at in (0, 4, 6):
        bad = [v, 2, 1, 32, v, v, f]
        bad[at] = None
        assert L.kjarni_hip_op_affine_repack(*bad) == E.NULL_POINTER, at
    for at in (1, 7):
        bad = [0, v, 2, 1, 32, None, 0, f]
        bad[at] = None
        assert L.kjarni_hip_op_affine_dequant(*bad) == E.NULL_POINTER, at
    assert not any(f)


def test_refusals_leave_the_outputs_alone():
    rng = np.random.default_rng(0)
    k = 256
    mats = [(t, T.random_blocks(t, 8, k, rng)) for t in (T.Q4_0, T.Q5_K, 8)]
    x = np.ones((9, k), F32)
    ys = [np.full((12, 8), 7.0, F32) for _ in range(3)]
    kw = dict(in_place=True, k=k)
    calls = [lambda: ops.affine_proj(3, mats[:1], x, 2, ys, **kw),                                     # no such mode
             lambda: ops.affine_proj(0, mats[:1], x, 9, ys, **kw),                                     # more than 8 rows
             lambda: ops.affine_proj(0, mats[:1], x, 0, ys, **kw),                                     # no rows
             lambda: ops.affine_proj(0, [(12, G.random_blocks(12, 8, k, rng))], x, 2, ys, **kw),       # Q4_K: qfused_kernel's
             lambda: ops.affine_proj(0, [(T.Q5_K, mats[1][1][:, :176])], x[:, :224], 2, ys, in_place=True, k=224),   # no whole Q5_K block
             lambda: ops.affine_proj(0, mats[:1], x, 2, ys, k=48, in_place=True),                      # k % 32
             lambda: ops.affine_proj(1, mats, x, 2, ys, row_off=11, **kw),                             # K / V rows past the outputs
             lambda: ops.affine_proj(1, mats, x, 2, ys, r=np.ones((2, 24), F32), **kw),                # residual with Q | K | V
             lambda: ops.affine_proj(2, mats[:2], x, 2, ys, bias=np.ones(8, F32), **kw),               # bias with SwiGLU
             lambda: ops.affine_proj(2, [mats[0], (8, mats[2][1][:4])], x, 2, ys, **kw),               # gate / up of different n
             lambda: ops.affine_proj(0, mats[:1], x, 2, ys, bias=np.ones(8, F32), bias_off=(1, 0, 0), **kw),   # bias_off + n > bias
             lambda: ops.affine_proj(0, mats[:1], x, 2, [np.full((12, 7), 7.0, F32)], **kw)]          # ldy < n
    for i, call in enumerate(calls):
        with pytest.raises(KjarniException) as e:
            call()
        assert e.value.code == E.INVALID_CONFIG, (i, str(e.value))
        assert all((y == 7.0).all() for y in ys), i
    for call in (lambda: ops.affine_dequant(8, mats[2][1], 8, k), lambda: ops.affine_dequant(T.Q4_0, mats[0][1], 8, k, ids=[]),
                 lambda: ops.affine_repack(12, mats[0][1], 8, k)):
        with pytest.raises(KjarniException) as e:
            call()
        assert e.value.code == E.INVALID_CONFIG


@pytest.mark.parametrize("name", list(T.NEW_TYPES))
def test_repack_is_the_documented_layout(name):
    t, n, k = T.NEW_TYPES[name], 5, 512
    blocks = T.random_blocks(t, n, k, np.random.default_rng(t))
    nib, high, ab = ops.affine_repack(t, blocks, n, k)
    # the layout in numpy: code of element e of a run = nibble (byte e % 16, high half from e = 16) | fifth bit e << 4; w = a q + b
    e = np.arange(32)
    runs = nib.reshape(n, k // 32, 16)
    q = np.where(e < 16, runs[:, :, e % 16] & 0xF, runs[:, :, e % 16] >> 4).astype(np.uint32)
    if name in ("Q5_0", "Q5_1", "Q5_K"):
        q |= ((high[:, :, None] >> e.astype(np.uint32)) & 1) << 4
    else:
        assert high is None
    w = (ab[:, :, 0:1].astype(np.float64) * q + ab[:, :, 1:2].astype(np.float64)).astype(F32).reshape(n, k)
    assert np.array_equal(w, T.dequantize(t, blocks, n, k))
