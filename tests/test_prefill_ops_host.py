"""The prefill entry points without a GPU: kjarni_hip_op_prefill_gemm and kjarni_hip_op_prefill_attention are declared, exported
and bound with their arity, answer NULL as declared, and refuse what their checks refuse -- INVALID_CONFIG from the argument
check, which comes before any GPU work, with every output still holding its sentinel.  Also the K-split rule restated in Python
against the table the GPU cases are built on, and the float64 GEMM reference against a naive triple loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from tests import prefill_ref64 as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {"kjarni_hip_op_prefill_gemm": 19, "kjarni_hip_op_prefill_attention": 17}
SENTINEL = 7.0


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
    used, route = C.c_int32(-5), C.c_int32(-5)
    args = [0, f, 32, 1, C.cast(f, C.c_void_p), 0, None, None, 0, 0, f, 4, None, 1, 4, 32, 0, C.byref(used), None]
    for at in (1, 4, 10, 17):                                            # a, w, y, ksplit_used
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_prefill_gemm(*bad) == E.NULL_POINTER
    args = [0, f, 64, 1, f, 4096, 64, f, 4096, 64, 0, 1, 64, 1, f, 64, C.byref(route)]
    for at in (1, 4, 7, 14, 16):                                         # q, k, v, ctx, route
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_prefill_attention(*bad) == E.NULL_POINTER
    assert used.value == -5 and route.value == -5 and not any(f)


# ---- refusals: the argument check comes first, so none of these needs a device ----------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _gemm(m=4, n=8, k=32, lda=None, ldy=None, ldr=None, residual=False, r_is_y=False, gate=False, a_rows=None, split=1, bf16=0,
          want_written=False):
    """A call with valid zero buffers for the sizes given; y, gate, ksplit_used and scratch_written start as sentinels that a
    refused call must leave alone.  Returns the error code."""
    lda = k if lda is None else lda
    ldy = n if ldy is None else ldy
    ldr = n if ldr is None else ldr
    rows = max(m, 1)
    a = np.zeros((rows if a_rows is None else max(a_rows, 1), max(lda, k, 1)), np.float32)
    w = np.zeros((max(n, 1), max(k, 1)), np.float32)
    y = np.full((rows, max(ldy, n, 1)), SENTINEL, np.float32)
    r = np.zeros((rows, max(ldr, n, 1)), np.float32) if residual else None
    g = np.full((rows, max(n, 1)), SENTINEL, np.float32) if gate else None
    used, written = C.c_int32(-5), C.c_int64(-5)
    rc = L.kjarni_hip_op_prefill_gemm(0, _p(a), lda, rows if a_rows is None else a_rows, w.ctypes.data_as(C.c_void_p), bf16, None, _p(r), ldr,
                                      int(r_is_y), _p(y), ldy, _p(g), m, n, k, split, C.byref(used), C.byref(written) if want_written else None)
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
], ids=str)
def test_gemm_refuses(kw):
    assert _gemm(**kw) == E.INVALID_CONFIG, kw


def test_gemm_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(m=0), dict(lda=36, ldy=12), dict(residual=True, ldr=12), dict(r_is_y=True, ldr=0, ldy=12), dict(gate=True),
               dict(split=0), dict(bf16=1), dict(a_rows=9), dict(want_written=True)):
        assert _gemm(**kw) in PASSES, kw
    assert _gemm() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


def _attention(rows=2, base=3, heads=2, d=16, kv_group=1, ldq=None, ldk=None, ldv=None, ldc=None, k_floats=None, v_floats=None):
    kvd = max(heads // max(kv_group, 1), 1) * max(d, 1)
    qd = max(heads, 1) * max(d, 1)
    ldq = qd if ldq is None else ldq
    ldc = qd if ldc is None else ldc
    ldk = kvd if ldk is None else ldk
    ldv = kvd if ldv is None else ldv
    keys = max(base + rows, 1)
    q = np.zeros((max(rows, 1), max(ldq, qd)), np.float32)
    k = np.zeros(keys * max(ldk, kvd), np.float32)
    v = np.zeros(keys * max(ldv, kvd), np.float32)
    ctx = np.full((max(rows, 1), max(ldc, qd)), SENTINEL, np.float32)
    route = C.c_int32(-5)
    rc = L.kjarni_hip_op_prefill_attention(0, _p(q), ldq, rows, _p(k), k.size if k_floats is None else k_floats, ldk, _p(v),
                                           v.size if v_floats is None else v_floats, ldv, base, heads, d, kv_group, _p(ctx), ldc, C.byref(route))
    if rc != E.OK:
        assert (ctx == SENTINEL).all() and route.value == -5, "a refused call wrote its output"
    return rc


@pytest.mark.parametrize("kw", [
    dict(d=8), dict(d=48), dict(d=96), dict(d=256), dict(d=0), dict(d=-64),
    dict(rows=0), dict(rows=-1), dict(base=-1), dict(kv_group=0), dict(kv_group=-1),
    dict(heads=3, kv_group=2), dict(heads=2, kv_group=4), dict(heads=0),
    dict(ldq=34), dict(ldk=34), dict(ldv=34), dict(ldc=34),              # not multiples of 4
    dict(ldq=28), dict(ldk=28), dict(ldv=28), dict(ldc=28),              # narrower than the heads
    dict(heads=4, kv_group=2, ldk=28),
    dict(k_floats=5 * 32 - 1), dict(v_floats=5 * 32 - 1),                # the last key row ends one float outside
    dict(ldk=36, k_floats=4 * 36 + 31), dict(ldv=36, v_floats=4 * 36 + 31),
], ids=str)
def test_attention_refuses(kw):
    assert _attention(**kw) == E.INVALID_CONFIG, kw


def test_attention_accepts_the_edges_of_its_check():
    for kw in (dict(), dict(base=0, rows=1), dict(heads=4, kv_group=2), dict(heads=14, kv_group=7), dict(ldq=36, ldk=36, ldv=40, ldc=44),
               dict(ldk=36, k_floats=4 * 36 + 32), dict(ldv=36, v_floats=4 * 36 + 32), dict(d=32), dict(d=64), dict(d=128)):
        assert _attention(**kw) in PASSES, kw


# ---- the K-split rule and the reference ---------------------------------------------------------------------------------------------------

# (M, N, K) -> (ksplit, workgroups, K tiles per slice): the table of tests/test_gpu_prefill_ops.py
TABLE = {
    (24, 64, 32): (1, 1, 1), (63, 60, 96): (1, 1, 3), (64, 64, 192): (1, 1, 6), (65, 68, 256): (2, 8, 4), (100, 132, 320): (2, 12, 5),
    (33, 64, 512): (4, 4, 4), (70, 196, 768): (4, 32, 6), (64, 128, 1024): (8, 16, 4), (65, 132, 1280): (8, 48, 5), (1, 4, 1024): (8, 8, 4),
    (129, 64, 1024): (8, 24, 4), (65, 4160, 1024): (4, 520, 8), (65, 16448, 256): (1, 514, 8), (24, 37, 1024): (1, 1, 32),
}


def test_the_split_rule_restated_gives_the_table():
    for shape, want in TABLE.items():
        assert P.geometry(*shape) == want, shape
    assert {v[0] for v in TABLE.values()} == {1, 2, 4, 8}
    assert all(P.ksplit_rule(*shape, scratch=False) == 1 for shape in TABLE)
    # the caps: 128 tiles still take 8 slices, 129 take 4; 512 tiles take 2, 513 none
    assert P.ksplit_rule(64, 128 * 64, 1024) == 8 and P.ksplit_rule(64, 129 * 64, 1024) == 4
    assert P.ksplit_rule(64, 512 * 64, 1024) == 2 and P.ksplit_rule(64, 513 * 64, 1024) == 1


def test_gemm64_against_a_naive_triple_loop():
    rng = np.random.default_rng(5)
    m, n, k = 5, 7, 32
    a, w = rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((n, k)).astype(np.float32)
    bias, r, gate = (rng.standard_normal(s).astype(np.float32) for s in ((n,), (m, n), (m, n)))
    w16 = ops.to_bf16(w)
    for bf16, wv in ((False, w.astype(np.float64)), (True, ops.bf16_to_f32(w16).astype(np.float64))):
        naive = np.zeros((m, n))
        for i in range(m):
            for j in range(n):
                acc = 0.0
                for c in range(k):
                    acc += float(a[i, c]) * float(wv[j, c])
                naive[i, j] = acc + float(bias[j]) + float(r[i, j])
        y, sw = P.gemm64(a, w16 if bf16 else w, bias, r, gate, bf16=bf16)
        assert np.abs(y - naive).max() < 1e-13
        silu = np.array([[float(gate[i, j]) / (1.0 + np.exp(-float(gate[i, j]))) for j in range(n)] for i in range(m)])
        assert np.abs(sw - silu * naive).max() < 1e-13
        assert np.array_equal(P.gemm64(a, w16 if bf16 else w, bias, r, bf16=bf16), y)
    assert np.abs(P.gemm64(a, w) - a.astype(np.float64) @ w.astype(np.float64).T).max() == 0
