"""Wide lanes, host side (no GPU): the new symbols are declared, exported and bound with their arities and answer NULL as
declared; the binding's mirror of the wide state has the native size; the two op hooks refuse bad arguments before any GPU
work, with every output untouched; and the prompt sets of tests/test_gpu_wide_lanes.py clear their gap preconditions in the
references alone.  (The refusals of the handle-taking entry points need a loaded decoder, hence a device: they are in the GPU
file.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import lanes_cases as LC
from tests import wide_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

WIDE_SYMBOLS = {
    "kjarni_hip_decoder_generate_wide": 14, "kjarni_hip_decoder_wide_begin": 3, "kjarni_hip_decoder_wide_prefill": 4,
    "kjarni_hip_decoder_wide_prefill_shared": 5, "kjarni_hip_decoder_wide_step": 5, "kjarni_hip_decoder_wide_cache_len": 2,
    "kjarni_hip_decoder_wide_capacity": 1, "kjarni_hip_decoder_wide_kv_rows": 7, "kjarni_hip_generator_set_wide_lanes": 2,
    "kjarni_hip_wide_state_size": 0, "kjarni_hip_op_wide_rope_scatter": 20, "kjarni_hip_op_wide_pick": 11,
}


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_wide_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in WIDE_SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/kjarni_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip() and a.strip() != "void"]), name
    # generate_wide has generate_batch's signature
    assert _ffi.SIGNATURES["kjarni_hip_decoder_generate_wide"] == _ffi.SIGNATURES["kjarni_hip_decoder_generate_batch"]
    assert decl["kjarni_hip_decoder_generate_wide"].split() == decl["kjarni_hip_decoder_generate_batch"].split()
    assert _ffi.SIGNATURES["kjarni_hip_decoder_wide_cache_len"][0] is C.c_int32


def test_the_state_mirror_has_the_native_size():
    assert C.sizeof(_ffi.KjarniHipWideState) == L.kjarni_hip_wide_state_size() == 64 * 4 * (6 + 16)
    st = _ffi.KjarniHipWideState()
    assert len(st.token) == len(st.pos) == len(st.live) == len(st.count) == len(st.limit) == len(st.n_stop) == len(st.stop) == 64
    assert len(st.stop[0]) == 16 and _ffi.KjarniHipWideState.stop.offset == 64 * 4 * 6


def test_null_handles_and_empty_batches():
    n_out = (C.c_size_t * 1)(7)
    off = (C.c_size_t * 2)(0, 1)
    new = (C.c_size_t * 1)(4)
    ids = (C.c_uint32 * 1)(5)
    cb = _ffi.KjarniBatchTokenCallbackFn()
    assert L.kjarni_hip_decoder_generate_wide(None, ids, off, 1, new, 1.0, 0, 0, 0, cb, None, None, 0, n_out) == E.NULL_POINTER
    assert n_out[0] == 7                                                 # nothing written
    assert L.kjarni_hip_decoder_wide_begin(None, 16, 0) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_wide_prefill(None, 0, ids, 1) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_wide_prefill_shared(None, 0, 0, ids, 1) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_wide_step(None, ids, None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_wide_cache_len(None, 0) == -1 and L.kjarni_hip_decoder_wide_capacity(None) == 0
    assert L.kjarni_hip_decoder_wide_kv_rows(None, 0, 0, 0, 0, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_wide_lanes(None, 16) == E.NULL_POINTER
    assert L.kjarni_hip_op_wide_rope_scatter(0, None, 8, 9, 1, 1, 2, None, None, 0.0, None, None, 1, None, None, 8, 1, None, None, 1) == E.NULL_POINTER
    assert L.kjarni_hip_op_wide_pick(0, None, 8, 8, 9, 0, None, None, 4, 8, 1) == E.NULL_POINTER


def _scatter_args(lanes=9, heads=2, kvh=1, d=8, cap=4, rows=5):
    width = (heads + 2 * kvh) * d
    return dict(qkv=np.full((lanes, width), 3.0, np.float32), n_heads=heads, n_kv_heads=kvh, head_dim=d,
                cos_t=np.ones((cap, d // 2), np.float32), sin_t=np.zeros((cap, d // 2), np.float32),
                k_cache=np.full((lanes, rows, kvh * d), 5.0, np.float32), v_cache=np.full((lanes, rows, kvh * d), 7.0, np.float32),
                capacity=cap, pos=np.zeros(lanes, np.int32), live=np.ones(lanes, np.int32))


@pytest.mark.parametrize("change,word", [
    (dict(qkv=np.zeros((65, 32), np.float32), k_cache=np.zeros((65, 5, 8), np.float32), v_cache=np.zeros((65, 5, 8), np.float32),
          pos=np.zeros(65, np.int32), live=np.ones(65, np.int32)), "lanes"),
    (dict(head_dim=7), "head"), (dict(head_dim=130), "head"), (dict(n_kv_heads=3), "head"),
    (dict(qkv=np.zeros((9, 31), np.float32)), "ld"),
    (dict(capacity=6), "lane_stride"),
    (dict(pos=np.array([0, -1] + [0] * 7, np.int32)), "pos[1]"),
    (dict(capacity=5, pos=np.array([4] + [0] * 8, np.int32)), "pos[0]"),                      # inside the capacity, outside the tables
    (dict(gamma_q=np.ones(8, np.float32)), "gamma"),
    (dict(gamma_q=np.ones(8, np.float32), gamma_k=np.ones(8, np.float32), rotate=False), "rotate"),
])
def test_the_scatter_hook_refuses_bad_arguments_before_any_gpu_work(change, word):
    a = _scatter_args()
    a.update(change)
    with pytest.raises(KjarniException) as e:                              # (no device is needed to get here)
        ops.wide_rope_scatter(**a)
    assert e.value.code == E.INVALID_CONFIG and word in e.value.message, e.value.message


def test_the_scatter_hook_leaves_its_outputs_untouched_on_a_refusal():
    a = _scatter_args()
    q, k, v = (np.ascontiguousarray(a[n]) for n in ("qkv", "k_cache", "v_cache"))
    f = lambda x: x.ctypes.data_as(_ffi._f32p)  # noqa: E731
    i = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    code = L.kjarni_hip_op_wide_rope_scatter(0, f(q), q.shape[1], 65, 2, 1, 8, None, None, 0.0, f(a["cos_t"]), f(a["sin_t"]), 4, f(k), f(v), 40, 4,
                                             i(a["pos"]), i(a["live"]), 1)
    assert code == E.INVALID_CONFIG
    assert (q == 3.0).all() and (k == 5.0).all() and (v == 7.0).all()


@pytest.mark.parametrize("kw,word", [
    (dict(lanes=65), "lanes"), (dict(lanes=9, first_lane=56), "lanes"), (dict(lanes=0), "lanes"), (dict(first_lane=-1), "lanes"),
    (dict(vocab=9), "vocab"), (dict(stride=0), "hist_stride"), (dict(n_stop=17), "n_stop[2]"), (dict(n_stop=-1), "n_stop[2]"),
    (dict(count=4), "count[2]"),
])
def test_the_pick_hook_refuses_bad_arguments_before_any_gpu_work(kw, word):
    st = _ffi.KjarniHipWideState()
    for l in range(64):
        st.live[l], st.limit[l] = 1, 100
    st.n_stop[2] = kw.get("n_stop", 0)
    st.count[2] = kw.get("count", 0)
    stride = kw.get("stride", 4)
    hist = np.full((64, max(stride, 1)), -7, np.int32)
    logits = np.zeros((64, 8), np.float32)
    before = bytes(st)
    code = L.kjarni_hip_op_wide_pick(0, logits.ctypes.data_as(_ffi._f32p), 8, kw.get("vocab", 8), kw.get("lanes", 9), kw.get("first_lane", 0),
                                     C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_int32)), stride, 16, 1)
    assert code == E.INVALID_CONFIG and word in _ffi.last_error(), _ffi.last_error()
    assert bytes(st) == before and (hist == -7).all()


@pytest.mark.parametrize("case", sorted(WC.SEEDS))
def test_the_prompt_sets_clear_their_gap_in_the_reference(case):
    """What tools/wide_seed_search.py found, asserted: 72 prompts, limits of 4..10, every step of every prompt GAP apart."""
    seed, cfg, t, ps, news = WC.case_set(case)
    assert len(ps) == len(news) == WC.N_PROMPTS == 72 and set(news) == set(range(4, 11))
    assert all(1 <= len(p) <= 39 and len(p) + m <= WC.LANE_CONTEXT for p, m in zip(ps, news))
    exp, gap = WC.reference_runs(case, cfg, t, ps, news)
    assert gap >= LC.GAP, f"{case}: the reference's two best logits come within {gap:.2e}"
    if case == "eos":
        ends = WC.stopped(exp, ps, news)
        assert len(ends) >= WC.EOS_MIN_STOPPED and len(set(ends.values())) >= 2, ends
    else:
        assert sum(len(e) for e in exp) >= 0.9 * sum(news)                 # (nearly) every limit is reached: lanes turn over by their limits


def test_the_moe_prompts_are_clear_in_the_reference():
    from tests import moe_fixture as M
    cfg = dict(M.MOE_SMALL)
    t = M.moe_tensors(cfg, M.MODEL_SEED)
    ps = WC.moe_prompts(cfg["vocab_size"])
    assert len(ps) == 20 and {len(p) for p in ps} == set(WC.MOE_LENGTHS)
    for i, p in enumerate(ps):
        assert len(WC.moe_clear_greedy(t, cfg, p, f"prompt {i}")) == WC.MOE_NEW
