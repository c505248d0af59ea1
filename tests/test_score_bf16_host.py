"""The bf16 matrix-core scoring head without a GPU: the counter's symbol, the op hooks' refusals of `fused`, and sp_split
(csrc/bf16_split.h) restated in numpy, which the GPU tests use to build inputs that only the third plane carries."""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from tests.test_gpu_score import _bf16_round
from tests.test_score_topk_abi import _declarations

L = kjarni_amd.lib()


def sp_split(x):
    """x f32 -> three bf16-representable f32 planes: round to nearest even, subtract, and again (the subtractions are exact)."""
    x = np.asarray(x, np.float32)
    p1 = _bf16_round(x)
    r = x - p1
    p2 = _bf16_round(r)
    return p1, p2, _bf16_round(r - p2)


def third_plane_case(m=65, k=96, vocab=200, seed=5):
    """X [m, k] = 2^14 * (1 + 2^-9 + n * 2^-19), n in 1..3: the three planes are 2^14, 2^5 and n / 32.  W [vocab, k] is +-1 with as many
    +1 as -1 in every 16 columns, so planes 1 and 2 cancel inside each k-step and logit = sum +-n / 32: every partial sum is a
    multiple of 1/32 below 2^19, exact in f32 in any order.  Returns X, W and the float64 logits."""
    rng = np.random.default_rng(seed)
    X = (np.float32(2.0 ** 14) * (1.0 + 2.0 ** -9 + rng.integers(1, 4, (m, k)) * 2.0 ** -19)).astype(np.float32)
    W = np.where(rng.permuted(np.tile(np.arange(16) < 8, (vocab, k // 16, 1)), axis=2), 1.0, -1.0).reshape(vocab, k).astype(np.float32)
    return X, W, X.astype(np.float64) @ W.astype(np.float64).T


def test_counter_symbol():
    name = "kjarni_hip_decoder_score_bf16_calls"
    assert [a.strip() for a in _declarations()[name].split(",")] == ["const KjarniHipDecoder* decoder"]
    restype, argtypes = _ffi.SIGNATURES[name]
    assert restype is C.c_uint64 and len(argtypes) == 1 and hasattr(L, name)
    assert L.kjarni_hip_decoder_score_bf16_calls(None) == 0
    L.kjarni_hip_decoder_set_score_fused(None, 2)                                        # NULL: nothing happens


@pytest.mark.parametrize("fused,bf16,field", [(2, 0, "bf16"), (3, 1, "fused"), (-1, 0, "fused")])
@pytest.mark.parametrize("topk", [False, True])
def test_op_hooks_refuse_fused_before_any_gpu_work(fused, bf16, field, topk):
    x, w = (C.c_float * 64)(), C.cast((C.c_float * 2048)(), C.c_void_p)
    lp, lse, tlp = (C.c_float * 2)(9.0, 9.0), (C.c_float * 2)(9.0, 9.0), (C.c_float * 2)(9.0, 9.0)
    tg, tid = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 2)(9, 9)
    if topk:
        code = L.kjarni_hip_op_score_head_topk(0, x, 2, 32, w, bf16, 64, tg, 0, fused, 1, lp, tid, tlp, lse)
    else:
        code = L.kjarni_hip_op_score_head(0, x, 2, 32, w, bf16, 64, tg, 0, fused, lp, tid, tlp, lse)
    assert code == E.INVALID_CONFIG and field in _ffi.last_error()
    assert list(lp) == list(lse) == list(tlp) == [9.0, 9.0] and list(tid) == [9, 9]


def test_split_planes_sum_back_exactly_and_the_third_carries_the_probe():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(1 << 16) * np.exp2(rng.integers(-20, 20, 1 << 16))).astype(np.float32)
    for v in (x, third_plane_case()[0]):
        planes = sp_split(v)
        assert all(np.array_equal(p, _bf16_round(p)) for p in planes)
        assert np.array_equal(sum(p.astype(np.float64) for p in planes), v.astype(np.float64))
    X, W, logits = third_plane_case()                                                      # ... and is carried by the third plane
    p1, p2, p3 = sp_split(X)
    assert (p1 == 2.0 ** 14).all() and (p2 == 2.0 ** 5).all() and (p3 != 0).all() and np.array_equal(W, _bf16_round(W))
    assert not ((p1 + p2).astype(np.float64) @ W.astype(np.float64).T).any()               # without plane 3 every logit is 0
    assert np.array_equal(logits, p3.astype(np.float64) @ W.astype(np.float64).T)
