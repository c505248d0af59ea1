"""The affine-32 prompt GEMM and its switch without a GPU: kjarni_hip_op_prefill_gemm_affine and the set_affine_matrix_cores entries
are declared, exported and bound with their arity and answer NULL as declared; the hook refuses what its check refuses --
INVALID_CONFIG from the argument check, which comes before a device is asked for, with every output still holding its sentinel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from tests import gguf_types_fixture as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
SYMBOLS = {"kjarni_hip_op_prefill_gemm_affine": (19, C.c_int32), "kjarni_hip_decoder_set_affine_matrix_cores": (2, None),
           "kjarni_hip_decoder_affine_matrix_cores": (1, C.c_int32), "kjarni_hip_chat_set_affine_matrix_cores": (2, C.c_int32),
           "kjarni_hip_generator_set_affine_matrix_cores": (2, C.c_int32)}
SENTINEL = 7.0


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    for name, (arity, restype) in SYMBOLS.items():
        assert name in decl and hasattr(L, name), name
        got_restype, argtypes = _ffi.SIGNATURES[name]
        assert got_restype is restype, name
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name
    from kjarni_amd import Chat, Generator, HipDecoder, ops
    assert all(callable(getattr(cls, "set_affine_matrix_cores")) for cls in (HipDecoder, Generator, Chat))
    assert callable(HipDecoder.affine_matrix_cores) and callable(ops.prefill_gemm_affine)


def test_null_handles_and_pointers():
    L.kjarni_hip_decoder_set_affine_matrix_cores(None, 1)                # a NULL handle is ignored
    assert L.kjarni_hip_decoder_affine_matrix_cores(None) == 0           # and reads as off
    assert L.kjarni_hip_chat_set_affine_matrix_cores(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_affine_matrix_cores(None, 1) == E.NULL_POINTER
    f = (C.c_float * 4096)()
    used = C.c_int32(-5)
    args = [0, f, 32, 1, C.cast(f, C.c_void_p), T.Q4_0, None, None, 0, 0, f, 4, None, 1, 4, 32, 0, C.byref(used), None]
    for at in (1, 4, 10, 17):                                            # a, blocks, y, ksplit_used
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_prefill_gemm_affine(*bad) == E.NULL_POINTER
    assert used.value == -5 and not any(f)


def _p(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _gemm(t=T.Q4_0, m=4, n=8, k=256, lda=None, ldy=None, ldr=None, residual=False, r_is_y=False, gate=False, a_rows=None, split=1,
          want_written=False):
    """A call with valid zero buffers for the sizes given; y, gate, ksplit_used and scratch_written start as sentinels that a refused
    call must leave alone.  Returns the error code."""
    lda, ldy, ldr = (k if lda is None else lda), (n if ldy is None else ldy), (n if ldr is None else ldr)
    rows = max(m, 1)
    a = np.zeros((rows if a_rows is None else max(a_rows, 1), max(lda, k, 1)), np.float32)
    be, bb = T.BLOCK.get(t, (32, 34))
    blocks = np.zeros((max(n, 1), (max(k, 1) + be - 1) // be * bb), np.uint8)
    y = np.full((rows, max(ldy, n, 1)), SENTINEL, np.float32)
    r = np.zeros((rows, max(ldr, n, 1)), np.float32) if residual else None
    g = np.full((rows, max(n, 1)), SENTINEL, np.float32) if gate else None
    used, written = C.c_int32(-5), C.c_int64(-5)
    rc = L.kjarni_hip_op_prefill_gemm_affine(0, _p(a), lda, rows if a_rows is None else a_rows, blocks.ctypes.data_as(C.c_void_p), t, None, _p(r), ldr,
                                             int(r_is_y), _p(y), ldy, _p(g), m, n, k, split, C.byref(used), C.byref(written) if want_written else None)
    if rc != E.OK:
        assert (y == SENTINEL).all() and (g is None or (g == SENTINEL).all()), "a refused call wrote its output"
        assert used.value == -5 and written.value == -5, "a refused call wrote its out-parameters"
    return rc


@pytest.mark.parametrize("kw", [
    dict(t=8), dict(t=12), dict(t=14), dict(t=0), dict(t=30),                                      # not one of the five types
    dict(k=48), dict(t=T.Q5_1, k=16), dict(t=T.Q5_K, k=288), dict(t=T.Q5_K, k=32),                 # k % 32, k % 256 for Q5_K
    dict(lda=258), dict(lda=262), dict(k=512, lda=256),                                            # lda % 4, lda < k
    dict(m=-1), dict(n=0), dict(k=0), dict(ldy=7), dict(ldy=4),
    dict(gate=True, n=8, ldy=12), dict(gate=True, n=6), dict(gate=True, n=6, ldy=8),
    dict(residual=True, ldr=7), dict(a_rows=3), dict(split=2), dict(split=0, want_written=True),
], ids=str)
def test_gemm_affine_refuses(kw):
    assert _gemm(**kw) == E.INVALID_CONFIG, kw


def test_gemm_affine_accepts_the_edges_of_its_check():
    passes = (E.OK, E.GPU_UNAVAILABLE)                                   # past the check: only the device may be missing
    for kw in [dict(t=t) for t in T.BLOCK] + [dict(k=32), dict(t=T.Q5_0, k=224), dict(m=0), dict(lda=260, ldy=12), dict(residual=True, ldr=12),
                                              dict(r_is_y=True, ldr=0, ldy=12), dict(gate=True), dict(split=0), dict(want_written=True)]:
        assert _gemm(**kw) in passes, kw
    assert _gemm() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)
