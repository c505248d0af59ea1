"""The FP8 prompt GEMM and its switch without a GPU: kjarni_hip_op_prefill_gemm_fp8 and the set_fp8_matrix_cores entries are
declared, exported and bound with their arity and answer NULL as declared; the hook refuses what its check refuses --
INVALID_CONFIG from the argument check, which comes before any GPU work, with every output still holding its sentinel; the
float64 reference against a naive triple loop; the K-split table the GPU cases are built on against the rule restated."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from tests import fp8_fixture as F
from tests import fp8_gemm_ref64 as R
from tests import prefill_ref64 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {"kjarni_hip_op_prefill_gemm_fp8": (21, C.c_int32), "kjarni_hip_decoder_set_fp8_matrix_cores": (2, None),
           "kjarni_hip_decoder_fp8_matrix_cores": (1, C.c_int32), "kjarni_hip_chat_set_fp8_matrix_cores": (2, C.c_int32),
           "kjarni_hip_generator_set_fp8_matrix_cores": (2, C.c_int32)}
SENTINEL = 7.0


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, (arity, restype) in SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/kjarni_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        got_restype, argtypes = _ffi.SIGNATURES[name]
        assert got_restype is restype, name
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name


def test_python_classes_carry_the_setter():
    from kjarni_amd import Chat, Generator, HipDecoder
    for cls in (HipDecoder, Generator, Chat):
        assert callable(getattr(cls, "set_fp8_matrix_cores")), cls
    assert callable(HipDecoder.fp8_matrix_cores)


def test_null_handles():
    L.kjarni_hip_decoder_set_fp8_matrix_cores(None, 1)                   # a NULL handle is ignored
    assert L.kjarni_hip_decoder_fp8_matrix_cores(None) == 0              # and reads as off
    assert L.kjarni_hip_chat_set_fp8_matrix_cores(None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_fp8_matrix_cores(None, 1) == E.NULL_POINTER


def test_null_pointers():
    f = (C.c_float * 4096)()
    used = C.c_int32(-5)
    args = [0, f, 32, 1, C.cast(f, C.c_void_p), f, 1, 1, None, None, 0, 0, f, 4, None, 1, 4, 32, 0, C.byref(used), None]
    for at in (1, 4, 5, 12, 19):                                         # a, codes, scale, y, ksplit_used
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_prefill_gemm_fp8(*bad) == E.NULL_POINTER
    assert used.value == -5 and not any(f)


# ---- refusals: the argument check comes first, so none of these needs a device ------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _gemm(m=4, n=8, k=32, lda=None, ldy=None, ldr=None, residual=False, r_is_y=False, gate=False, a_rows=None, split=1, scale_shape=(1, 1),
          nan_at=None, nan_code=0x7F, want_written=False):
    """A call with valid zero buffers for the sizes given; y, gate, ksplit_used and scratch_written start as sentinels that a
    refused call must leave alone.  Returns the error code."""
    lda = k if lda is None else lda
    ldy = n if ldy is None else ldy
    ldr = n if ldr is None else ldr
    rows = max(m, 1)
    a = np.zeros((rows if a_rows is None else max(a_rows, 1), max(lda, k, 1)), np.float32)
    codes = np.zeros((max(n, 1), max(k, 1)), np.uint8)
    if nan_at is not None:
        codes[nan_at] = nan_code
    scale = np.ones(max(int(np.prod(np.abs(scale_shape))), 1), np.float32)
    y = np.full((rows, max(ldy, n, 1)), SENTINEL, np.float32)
    r = np.zeros((rows, max(ldr, n, 1)), np.float32) if residual else None
    g = np.full((rows, max(n, 1)), SENTINEL, np.float32) if gate else None
    used, written = C.c_int32(-5), C.c_int64(-5)
    rc = L.kjarni_hip_op_prefill_gemm_fp8(0, _p(a), lda, rows if a_rows is None else a_rows, codes.ctypes.data_as(C.c_void_p), _p(scale),
                                          scale_shape[0], scale_shape[1], None, _p(r), ldr, int(r_is_y), _p(y), ldy, _p(g), m, n, k, split,
                                          C.byref(used), C.byref(written) if want_written else None)
    if rc != E.OK:
        assert (y == SENTINEL).all() and (g is None or (g == SENTINEL).all()), "a refused call wrote its output"
        assert used.value == -5 and written.value == -5, "a refused call wrote its out-parameters"
    return rc


PASSES = (E.OK, E.GPU_UNAVAILABLE)   # past the check: only the device may be missing


@pytest.mark.parametrize("kw", [
    dict(k=48), dict(k=16), dict(k=33, lda=36),                          # k % 32
    dict(lda=34), dict(lda=38),                                          # lda % 4
    dict(m=-1), dict(n=0), dict(n=-4), dict(k=0), dict(k=-32),
    dict(gate=True, n=8, ldy=12), dict(gate=True, n=6), dict(gate=True, n=6, ldy=8),
    dict(ldy=7), dict(ldy=4), dict(lda=28), dict(k=64, lda=32),          # ldy < n, lda < k
    dict(residual=True, ldr=7), dict(residual=True, ldr=4),              # ldr < n
    dict(a_rows=3), dict(split=2), dict(split=0, want_written=True),
    # scale shapes that fit no kind
    dict(scale_shape=(2, 1)), dict(scale_shape=(1, 2)), dict(scale_shape=(8, 2)), dict(scale_shape=(0, 0)), dict(scale_shape=(-1, 1)),
    dict(n=200, k=256, scale_shape=(1, 2)), dict(n=200, k=256, scale_shape=(2, 1)), dict(n=200, k=256, scale_shape=(3, 2)),
    dict(n=200, k=160, scale_shape=(2, 1)), dict(n=200, k=160, scale_shape=(2, 2)),     # block scales need k % 128 == 0
    # NaN codes, first, last and in between
    dict(nan_at=(0, 0)), dict(nan_at=(7, 31)), dict(nan_at=(3, 9), nan_code=0xFF),
], ids=str)
def test_gemm_fp8_refuses(kw):
    assert _gemm(**kw) == E.INVALID_CONFIG, kw


def test_gemm_fp8_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(m=0), dict(lda=36, ldy=12), dict(residual=True, ldr=12), dict(r_is_y=True, ldr=0, ldy=12), dict(gate=True),
               dict(split=0), dict(a_rows=9), dict(want_written=True), dict(scale_shape=(8, 1)), dict(n=200, k=256, scale_shape=(2, 2)),
               dict(n=200, k=256, scale_shape=(200, 1)), dict(n=128, k=128, scale_shape=(1, 1)), dict(nan_at=(2, 2), nan_code=0x7E)):
        assert _gemm(**kw) in PASSES, kw
    assert _gemm() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


# ---- the reference and the split table ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", F.KINDS)
def test_reference_against_a_naive_triple_loop(kind):
    rng = np.random.default_rng(5)
    m, n, k = 3, 130, 256                                                # two rows of blocks, two columns of blocks
    a = rng.standard_normal((m, k)).astype(np.float32)
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    s2 = np.asarray(scale, np.float32).reshape(F.scale_shape(kind, n, k))
    bias, r, gate = (rng.standard_normal(s).astype(np.float32) for s in ((n,), (m, n), (m, n)))
    naive = np.zeros((m, n))
    for i in range(m):
        for j in range(n):
            acc = 0.0
            for c in range(k):
                s = s2[j // 128, c // 128] if kind == "block" else (s2[j, 0] if kind == "channel" else s2[0, 0])
                acc += float(a[i, c]) * (float(F.TABLE[codes[j, c]]) * float(s))
            naive[i, j] = acc + float(bias[j]) + float(r[i, j])
    y, sw = R.gemm64(a, codes, scale, kind, bias, r, gate)
    assert np.abs(y - naive).max() < 1e-13
    silu = gate.astype(np.float64) / (1.0 + np.exp(-gate.astype(np.float64)))
    assert np.abs(sw - silu * naive).max() < 1e-13
    assert np.array_equal(R.weights64(codes, scale, kind).astype(np.float32), F.dequantize(codes, scale, kind))   # the fixture's f32 product


# (M, N, K) -> ksplit: the shapes of tests/test_gpu_fp8_gemm.py, by hand
TABLE = {(63, 60, 96): 1, (64, 64, 192): 1, (65, 68, 256): 2, (33, 64, 384): 2, (65, 200, 384): 2, (33, 64, 512): 4, (70, 196, 768): 4,
         (64, 128, 1024): 8, (1, 4, 1024): 8, (24, 37, 1024): 1, (65, 4160, 1024): 4, (9, 200, 512): 4, (64, 200, 512): 4, (256, 64, 256): 2,
         (130, 200, 128): 1, (130, 200, 2048): 8, (130, 200, 8192): 8, (65, 136, 1024): 8}


def test_the_split_rule_restated_gives_the_table():
    for shape, want in TABLE.items():
        assert P.ksplit_rule(*shape) == want, shape
        assert P.ksplit_rule(*shape, scratch=False) == 1
    assert P.ksplit_rule(33, 64, 384) == 2 and 384 // 2 == 192 and 192 % 128 == 64      # the second slice starts inside block 1
    from tests.test_gpu_fp8_gemm import SPLIT_TABLE
    assert all(TABLE[(m, n, k)] == want for m, n, k, want in SPLIT_TABLE)
