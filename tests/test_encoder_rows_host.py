"""The encoder's packed-row entry points without a GPU: the nine new symbols are declared, exported and bound with their arity,
answer NULL as declared, and refuse what their checks refuse -- INVALID_CONFIG before a device is asked for, with every output
still holding its sentinel.  Also launch_attention's route rule restated in Python (tests/encoder_rows_ref64.py) against a table
worked out by hand and against attention_route itself over a sweep of arguments, and the references against hand-computed cases
and the oracle's attention, embedding and mean pool on padded inputs."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from oracle import oracle as O
from tests import encoder_rows_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
F32 = np.float32
I32P = C.POINTER(C.c_int32)

SYMBOLS = {"kjarni_hip_op_mask_lengths": 5, "kjarni_hip_op_pack_index": 7, "kjarni_hip_op_encoder_embed": 20, "kjarni_hip_op_encoder_rope": 9,
           "kjarni_hip_op_attention_packed": 11, "kjarni_hip_op_pool_packed": 9, "kjarni_hip_op_small_linear": 9, "kjarni_hip_op_row_softmax": 6,
           "kjarni_hip_attention_route": 7}
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


def test_the_binding_names_the_kernels_as_the_reference_does():
    assert (ops.ATTN_NOTHING, ops.ATTN_SPLIT, ops.ATTN_PIPE_PADDED, ops.ATTN_PIPE_PACKED, ops.ATTN_PIPE_SHORT, ops.ATTN_CHUNKED, ops.ATTN_GENERIC) == \
        (R.NOTHING, R.SPLIT, R.PIPE_PADDED, R.PIPE_PACKED, R.PIPE_SHORT, R.CHUNKED, R.GENERIC)
    assert (ops.POOL_MEAN, ops.POOL_CLS, ops.POOL_MAX, ops.POOL_LAST) == (R.POOL_MEAN, R.POOL_CLS, R.POOL_MAX, R.POOL_LAST)
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    for name, v in (("NOTHING", 0), ("SPLIT", 1), ("PIPE_PADDED", 2), ("PIPE_PACKED", 3), ("PIPE_SHORT", 4), ("CHUNKED", 5), ("GENERIC", 6)):
        assert re.search(rf"KJARNI_HIP_ATTN_{name} = {v}\b", header), name


def _f(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _u(a):
    return None if a is None else a.ctypes.data_as(_ffi._u32p)


def _i(a):
    return None if a is None else a.ctypes.data_as(I32P)


def _untouched(rc, *outs):
    if rc != E.OK:
        for o in outs:
            assert (o == o.dtype.type(SENTINEL)).all(), "a refused call wrote its output"
    return rc


# ---- one call of every hook on valid sentinel buffers for the sizes given ---------------------------------------------------------

def _lengths(B=2, S=4):
    out = np.full(max(B, 1), int(SENTINEL), np.uint32)
    return _untouched(L.kjarni_hip_op_mask_lengths(0, _u(np.ones((max(B, 1), max(S, 1)), np.uint32)), B, S, _u(out)), out)


def _pack(mask=((1, 1, 0, 0), (1, 0, 1, 1)), cu=(0, 2, 5), capacity=5):
    m = np.array(mask, np.uint32)
    out = np.full(max(capacity, 1), int(SENTINEL), np.int32)
    return _untouched(L.kjarni_hip_op_pack_index(0, _u(m), _i(np.array(cu, np.int32)), m.shape[0], m.shape[1], _i(out), capacity), out)


def _embed(rows=3, B=2, S=3, H=8, vocab=5, max_pos=4, type_vocab=2, pos=True, typ=True, type_ids=None, gamma=False, beta=None, tok_src=None,
           pos_offset=0):
    beta = gamma if beta is None else beta
    ids = np.zeros((max(B, 1), max(S, 1)), np.uint32)
    ty = None if type_ids is None else np.array(type_ids, np.uint32).reshape(ids.shape)
    tb = lambda n: np.zeros((max(n, 1), max(H, 1)), F32)  # noqa: E731
    vec = np.ones(max(H, 1), F32)
    ts = None if tok_src is None else np.array(tok_src, np.int32)
    out = np.full((max(rows, 1), max(H, 1)), SENTINEL, F32)
    rc = L.kjarni_hip_op_encoder_embed(0, _u(ids), _u(ty), _f(tb(vocab)), _f(tb(max_pos)) if pos else None, _f(tb(type_vocab)) if typ else None,
                                       _f(vec) if gamma else None, _f(vec) if beta else None, 1e-5, rows, B, S, H, vocab, max_pos, type_vocab,
                                       pos_offset, 0, _i(ts), _f(out))
    return _untouched(rc, out)


def _rope(rows=3, S=4, heads=2, d=4, tok_src=None):
    q = np.full((max(rows, 1), 3 * max(heads, 1) * max(d, 1)), SENTINEL, F32)
    t = np.zeros((max(S, 1), max(d, 1)), F32)
    ts = None if tok_src is None else np.array(tok_src, np.int32)
    return _untouched(L.kjarni_hip_op_encoder_rope(0, _f(q), _f(t), _f(t), rows, S, heads, d, _i(ts)), q)


def _attn(cu=(0, 2, 5), max_len=3, heads=2, d=32, buffer_rows=5):
    H = max(heads, 1) * max(d, 1)
    qkv = np.zeros((max(buffer_rows, 1), 3 * H), F32)
    ctx = np.full((max(buffer_rows, 1), H), SENTINEL, F32)
    route = np.full(2, int(SENTINEL), np.int32)
    rc = L.kjarni_hip_op_attention_packed(0, _f(qkv), _i(np.array(cu, np.int32)), len(cu) - 1, max_len, heads, d, -1e9, _f(ctx), buffer_rows, _i(route))
    return _untouched(rc, ctx, route)


def _pool(cu=(0, 2, 5), seq=3, H=8, pooling=0):
    hs = np.zeros((max(cu[-1], 1), max(H, 1)), F32)
    out = np.full((len(cu) - 1, max(H, 1)), SENTINEL, F32)
    return _untouched(L.kjarni_hip_op_pool_packed(0, _f(hs), _i(np.array(cu, np.int32)), len(cu) - 1, seq, H, pooling, 0, _f(out)), out)


def _linear(rows=3, k=8, n=2, ld=None):
    ld = k if ld is None else ld
    out = np.full((max(rows, 1), max(n, 1)), SENTINEL, F32)
    feat, w = np.zeros((max(rows, 1), max(ld, k, 1)), F32), np.zeros((max(n, 1), max(k, 1)), F32)
    return _untouched(L.kjarni_hip_op_small_linear(0, _f(feat), ld, _f(w), None, rows, k, n, _f(out)), out)


def _softmax(rows=3, n=2):
    out = np.full((max(rows, 1), max(n, 1)), SENTINEL, F32)
    return _untouched(L.kjarni_hip_op_row_softmax(0, _f(np.zeros_like(out)), rows, n, 0, _f(out)), out)


REFUSED = [
    (_lengths, dict(B=0)), (_lengths, dict(S=0)), (_lengths, dict(B=-1)), (_lengths, dict(B=(1 << 20) + 1)),
    # pack_index: the kernel writes tok_src + cu[b] unchecked
    (_pack, dict(cu=(1, 3, 6), capacity=8)),          # does not start at 0
    (_pack, dict(cu=(0, 2, 1))),                      # decreases
    (_pack, dict(cu=(0, 3, 5))),                      # steps differ from the mask's kept counts (3 + 2 for 2 + 3)
    (_pack, dict(cu=(0, 2, 4))),                      # the last sentence one short
    (_pack, dict(capacity=4)),                        # ends beyond capacity
    (_pack, dict(capacity=-1)),
    (_pack, dict(mask=((2, 0xFFFFFFFF, 0, 0), (1, 0, 1, 1)), cu=(0, 1, 4))),   # any non-zero value is a kept token
    # encoder_embed
    (_embed, dict(tok_src=(0, 6, 1))), (_embed, dict(tok_src=(0, -1, 1))), (_embed, dict(tok_src=(0, 1, 1 << 30))),   # outside [0, B * S)
    (_embed, dict(type_ids=(0, 1, 2, 0, 0, 0))), (_embed, dict(type_ids=(0, 0, 0, 0, 0, 0xFFFFFFFF))),               # a type id >= type_vocab
    (_embed, dict(gamma=True, beta=False)),                                                                          # gamma without beta
    (_embed, dict(max_pos=0)), (_embed, dict(max_pos=-3)), (_embed, dict(pos=False, max_pos=-1)),                     # pos with max_pos <= 0
    (_embed, dict(rows=7)), (_embed, dict(rows=0)), (_embed, dict(H=0)), (_embed, dict(H=8200)), (_embed, dict(vocab=0)), (_embed, dict(type_vocab=0)),
    (_embed, dict(pos_offset=-1)), (_embed, dict(S=0)), (_embed, dict(B=0)),
    # encoder_rope
    (_rope, dict(d=5)), (_rope, dict(d=0)), (_rope, dict(d=258)), (_rope, dict(heads=0)), (_rope, dict(S=0)), (_rope, dict(rows=0)),
    (_rope, dict(tok_src=(0, -1, 2))),
    # attention_packed: extents come from len - 1, grids from max_len
    (_attn, dict(cu=(1, 3, 5))), (_attn, dict(cu=(0, 2, 2))), (_attn, dict(cu=(0, 3, 2))), (_attn, dict(cu=(0, 0, 5), max_len=5)),   # not strictly increasing from 0
    (_attn, dict(max_len=2)),                                                                                                    # a length above max_len
    (_attn, dict(buffer_rows=4)),                                                                                                # cu[B] > buffer_rows
    (_attn, dict(heads=0)), (_attn, dict(d=0)), (_attn, dict(d=257)), (_attn, dict(max_len=0)), (_attn, dict(max_len=8193)), (_attn, dict(buffer_rows=0)),
    (_attn, dict(cu=(0,))),
    # pool_packed: the same cu checks, hidden <= 1024
    (_pool, dict(cu=(1, 3, 5))), (_pool, dict(cu=(0, 2, 2))), (_pool, dict(cu=(0, 3, 2))), (_pool, dict(seq=2)), (_pool, dict(H=1025)), (_pool, dict(H=0)),
    (_pool, dict(pooling=4)), (_pool, dict(pooling=-1)), (_pool, dict(seq=0)),
    (_linear, dict(rows=0)), (_linear, dict(k=0)), (_linear, dict(n=0)), (_linear, dict(ld=7)), (_linear, dict(n=4097)),
    (_softmax, dict(rows=0)), (_softmax, dict(n=0)), (_softmax, dict(n=4097)),
]


@pytest.mark.parametrize("call,kw", REFUSED, ids=lambda v: v.__name__ if callable(v) else str(v))
def test_refused_before_any_gpu_work_with_the_outputs_untouched(call, kw):
    assert call(**kw) == E.INVALID_CONFIG, kw


def test_the_edges_of_the_checks_are_accepted():
    for call, kw in ((_lengths, {}), (_lengths, dict(B=1, S=1)), (_pack, {}), (_pack, dict(capacity=9)),
                     (_pack, dict(mask=((0, 0), (0, 0)), cu=(0, 0, 0), capacity=0)),
                     (_pack, dict(mask=((2, 0xFFFFFFFF, 0, 0), (1, 0, 1, 1)), cu=(0, 2, 5))),
                     (_embed, {}), (_embed, dict(rows=6)), (_embed, dict(tok_src=(5, 0, 5))), (_embed, dict(type_ids=(0, 1, 1, 0, 1, 0))),
                     (_embed, dict(gamma=True)), (_embed, dict(gamma=False, beta=True)), (_embed, dict(pos=False, max_pos=0)), (_embed, dict(typ=False, type_vocab=0)),
                     (_embed, dict(typ=False, type_ids=(9, 9, 9, 9, 9, 9))), (_embed, dict(pos_offset=9)), (_embed, dict(H=6)), (_embed, dict(rows=9, tok_src=(0,) * 9)),
                     (_rope, {}), (_rope, dict(d=2)), (_rope, dict(tok_src=(0, 1 << 30, 2))), (_rope, dict(rows=9)),
                     (_attn, {}), (_attn, dict(max_len=128)), (_attn, dict(buffer_rows=133)), (_attn, dict(d=48)), (_attn, dict(cu=(0, 1), max_len=1)),
                     (_pool, {}), (_pool, dict(seq=512)), (_pool, dict(H=1024)), (_pool, dict(pooling=3)),
                     (_linear, {}), (_linear, dict(ld=20)), (_linear, dict(k=1, n=1, rows=1)), (_softmax, {}), (_softmax, dict(rows=1, n=1))):
        assert call(**kw) in PASSES, (call.__name__, kw)
    assert _attn() == (E.OK if kjarni_amd.device_count() > 0 else E.GPU_UNAVAILABLE)


def test_null_pointers():
    f = np.full(64, SENTINEL, F32)
    u, i = f.view(np.uint32), f.view(np.int32)
    cu = np.array([0, 1], np.int32)
    calls = [
        (L.kjarni_hip_op_mask_lengths, [0, _u(u), 1, 1, _u(u)], (1, 4)),
        (L.kjarni_hip_op_pack_index, [0, _u(u), _i(cu), 1, 1, _i(i), 4], (1, 2, 5)),
        (L.kjarni_hip_op_encoder_embed, [0, _u(u), None, _f(f), None, None, None, None, 0.0, 1, 1, 1, 4, 1, 0, 0, 0, 0, None, _f(f)], (1, 3, 19)),
        (L.kjarni_hip_op_encoder_rope, [0, _f(f), _f(f), _f(f), 1, 1, 1, 2, None], (1, 2, 3)),
        (L.kjarni_hip_op_attention_packed, [0, _f(f), _i(cu), 1, 1, 1, 4, 0.0, _f(f), 1, _i(i)], (1, 2, 8, 10)),
        (L.kjarni_hip_op_pool_packed, [0, _f(f), _i(cu), 1, 1, 4, 0, 0, _f(f)], (1, 2, 8)),
        (L.kjarni_hip_op_small_linear, [0, _f(f), 4, _f(f), None, 1, 4, 1, _f(f)], (1, 3, 8)),
        (L.kjarni_hip_op_row_softmax, [0, _f(f), 1, 4, 0, _f(f)], (1, 5)),
        (L.kjarni_hip_attention_route, [1, 1, 1, 32, 1, 0, _i(i)], (6,)),
    ]
    for fn, args, nullable in calls:
        for at in nullable:
            bad = list(args)
            bad[at] = None
            assert fn(*bad) == E.NULL_POINTER, (fn.__name__, at)
    assert (f == SENTINEL).all()


# ---- the route ----------------------------------------------------------------------------------------------------------------------

ROUTE_TABLE = [
    # (batch, seq / longest, heads, head_dim, aligned, packed) -> (kernel, grid), worked out by hand from attention.hip
    ((0, 64, 12, 32, True, True), (R.NOTHING, 0)), ((4, 0, 12, 32, True, False), (R.NOTHING, 0)),
    ((32, 64, 4, 32, True, True), (R.SPLIT, 0)),                 # 128 items
    ((43, 64, 3, 32, True, True), (R.PIPE_PACKED, 129)),         # 129 items
    ((1, 128, 12, 64, True, True), (R.SPLIT, 0)), ((10, 128, 12, 32, True, False), (R.SPLIT, 0)),
    ((11, 128, 12, 32, True, False), (R.PIPE_PADDED, 132)), ((11, 96, 12, 32, True, False), (R.PIPE_SHORT, 132)),
    ((11, 97, 12, 32, True, False), (R.PIPE_PADDED, 132)), ((11, 96, 12, 32, True, True), (R.PIPE_PACKED, 132)),
    ((11, 97, 12, 64, True, True), (R.PIPE_PACKED, 132)), ((11, 128, 12, 64, True, True), (R.PIPE_PACKED, 132)),
    ((11, 129, 12, 64, True, True), (R.CHUNKED, 0)), ((1, 129, 1, 32, True, True), (R.CHUNKED, 0)), ((11, 129, 12, 32, True, False), (R.CHUNKED, 0)),
    ((33, 100, 4, 32, True, True), (R.PIPE_PACKED, 132)),
    ((64, 128, 12, 32, True, True), (R.PIPE_PACKED, 768)), ((65, 128, 12, 32, True, True), (R.PIPE_PACKED, 768)),     # 768 / 780 items: the cap at head_dim 32
    ((154, 60, 5, 32, True, True), (R.PIPE_PACKED, 768)), ((153, 60, 5, 32, True, True), (R.PIPE_PACKED, 765)),
    ((171, 128, 3, 64, True, True), (R.PIPE_PACKED, 512)), ((170, 128, 3, 64, True, True), (R.PIPE_PACKED, 510)),     # the cap at head_dim 64
    ((4096, 128, 12, 64, True, False), (R.PIPE_PADDED, 512)), ((4096, 40, 12, 32, True, False), (R.PIPE_SHORT, 768)),
    ((4, 64, 8, 48, True, True), (R.GENERIC, 0)), ((4096, 200, 12, 48, True, False), (R.GENERIC, 0)), ((4, 64, 8, 16, True, True), (R.GENERIC, 0)),
    ((4, 64, 12, 32, False, True), (R.GENERIC, 0)), ((4096, 64, 12, 64, False, False), (R.GENERIC, 0)), ((4, 300, 12, 64, False, True), (R.GENERIC, 0)),
]


@pytest.mark.parametrize("args,want", ROUTE_TABLE, ids=str)
def test_the_restated_route_against_the_table(args, want):
    assert R.attention_route(*args) == want
    assert ops.attention_route(*args) == want


def test_the_restated_route_against_attention_route_over_a_sweep():
    n = 0
    for batch, seq, heads, d, aligned, packed in itertools.product(
            (0, 1, 2, 10, 11, 32, 33, 42, 43, 64, 65, 128, 129, 170, 171, 256, 257, 768, 769, 4096, 70000), (0, 1, 31, 32, 95, 96, 97, 127, 128, 129, 200, 512),
            (1, 2, 3, 4, 5, 7, 12, 16), (8, 16, 31, 32, 33, 48, 63, 64, 65, 128), (False, True), (False, True)):
        assert ops.attention_route(batch, seq, heads, d, aligned, packed) == R.attention_route(batch, seq, heads, d, aligned, packed), \
            (batch, seq, heads, d, aligned, packed)
        n += 1
    for items in range(1, 1600):                                  # every item count across both caps and the small-call limit
        for d in (32, 64):
            assert ops.attention_route(items, 64, 1, d, True, True) == R.attention_route(items, 64, 1, d, True, True), (items, d)
            n += 1
    assert n > 80000


def test_route_refuses_nonsense_sizes():
    r = np.full(2, int(SENTINEL), np.int32)
    for args in ((1, 1, 0, 32), (1, 1, 1, 0), (1, 1, -1, 32)):
        assert L.kjarni_hip_attention_route(*args, 1, 0, _i(r)) == E.INVALID_CONFIG
    assert (r == int(SENTINEL)).all()


# ---- the references -----------------------------------------------------------------------------------------------------------------

def test_lengths_and_index_by_hand():
    mask = np.array([[1, 1, 0, 0], [1, 0, 1, 1], [0, 1, 1, 0], [0, 0, 0, 0], [1, 2, 0, 0], [1, 0xFFFFFFFF, 1, 1]], np.uint32)
    B31 = 0x80000000
    assert R.mask_lengths(mask).tolist() == [2, 3, 2 | B31, 0 | B31, 2 | B31, 4 | B31]
    cu, src = R.pack_index(mask)
    assert cu.tolist() == [0, 2, 5, 7, 7, 9, 13]
    assert src.tolist() == [0, 1, 4, 6, 7, 9, 10, 16, 17, 20, 21, 22, 23]


def test_attention_reference_by_hand_and_against_the_oracle():
    # one head of width 2, a sentence of two tokens whose scores are (0, 0) and (ln 3 sqrt 2 / sqrt 2, 0): probabilities 1/2, 1/2 and 3/4, 1/4
    qkv = np.zeros((3, 6), np.float64)
    qkv[1, 0] = np.log(3.0) * np.sqrt(2.0)
    qkv[0, 2], qkv[0, 4:6], qkv[1, 4:6] = 1.0, (4.0, 8.0), (0.0, -8.0)
    qkv[2, 4:6] = (5.0, 6.0)                                       # a sentence of one token returns its own V
    ctx = R.attention_packed(qkv, [2, 1], 1, 2)
    assert np.allclose(ctx, [[2.0, 0.0], [3.0, 4.0], [5.0, 6.0]], atol=1e-14)
    rng = np.random.default_rng(0)
    B, S, heads, d = 3, 9, 2, 8
    lens = [9, 4, 1]
    x = rng.standard_normal((B, S, 3 * heads * d)).astype(F32)
    mask = np.array([[1] * n + [0] * (S - n) for n in lens], np.uint32)
    H = heads * d
    want = O.attention(x[..., :H], x[..., H:2 * H], x[..., 2 * H:], mask, heads)
    packed = np.concatenate([x[b, :n] for b, n in enumerate(lens)])
    got = R.attention_packed(packed, lens, heads, d)
    at = 0
    for b, n in enumerate(lens):
        assert np.abs(got[at:at + n] - want[b, :n]).max() < 2e-6
        at += n


def test_embedding_reference_against_the_oracle_and_by_hand():
    rng = np.random.default_rng(1)
    B, S, H, V, P, T = 2, 5, 8, 7, 6, 2
    word, pos, typ = (rng.standard_normal(s).astype(F32) for s in ((V, H), (P, H), (T, H)))
    ids = rng.integers(0, V, (B, S)).astype(np.uint32)
    ids[0, 1], ids[1, 4] = V, 0xFFFFFFFF
    tys = rng.integers(0, T, (B, S)).astype(np.uint32)
    for off, scale in ((0, False), (2, True)):
        want = O.embed(ids, tys, word, pos, typ, pos_offset=off, scale=scale).reshape(B * S, H)
        got = R.embed_f32(ids, word, pos, typ, tys, S, V, P, T, off, scale, np.arange(B * S))
        assert np.abs(got - want).max() <= 1e-6
    got = R.embed_f32(ids, word, pos, None, None, S, V, P, 0, 2, False, [6, 9, 1])
    assert np.array_equal(got[0], word[ids[1, 1]] + pos[3]) and np.array_equal(got[1], np.zeros(H, F32)) and np.array_equal(got[2], pos[3])
    x = np.array([[1.0, 2.0, 3.0, 6.0]])
    assert np.allclose(R.layer_norm(x, np.full(4, 2.0), np.ones(4), 0.0), 1 + 2 * (x - 3.0) / np.sqrt(3.5), atol=1e-14)
    assert np.abs(R.layer_norm(got, np.ones(H), np.zeros(H), 1e-5) - O.layer_norm(got, np.ones(H, F32), np.zeros(H, F32), 1e-5)).max() < 1e-5


def test_rope_reference_by_hand():
    qkv = np.arange(1, 13, dtype=F32).reshape(1, 12)               # heads 1, head_dim 4: pairs (x0, x2), (x1, x3)
    cos, sin = np.array([[9, 9, 9, 9], [0.5, 0.25, 9, 9]], F32), np.array([[9, 9, 9, 9], [2.0, 4.0, 9, 9]], F32)
    got = R.rope_f32(qkv, cos, sin, 1, 4, [1])
    assert got[0].tolist() == [1 * 0.5 - 3 * 2, 2 * 0.25 - 4 * 4, 1 * 2 + 3 * 0.5, 2 * 4 + 4 * 0.25,
                               5 * 0.5 - 7 * 2, 6 * 0.25 - 8 * 4, 5 * 2 + 7 * 0.5, 6 * 4 + 8 * 0.25, 9, 10, 11, 12]


def test_pool_references_by_hand_and_against_the_oracle():
    hs = np.array([[1, -2], [3, 4], [0, 0], [-5, 6], [7, 8], [0, 0]], np.float64)
    lens = [2, 1, 2, 1]
    assert R.pool_packed(hs, lens, R.POOL_MEAN, False).tolist() == [[2, 1], [0, 0], [1, 7], [0, 0]]
    assert R.pool_packed(hs, lens, R.POOL_CLS, False).tolist() == [[1, -2], [0, 0], [-5, 6], [0, 0]]
    assert R.pool_packed(hs, lens, R.POOL_MAX, False).tolist() == [[3, 4], [0, 0], [7, 8], [0, 0]]
    assert R.pool_packed(hs, lens, R.POOL_LAST, False).tolist() == [[3, 4], [0, 0], [7, 8], [0, 0]]
    n = R.pool_packed(hs, lens, R.POOL_LAST, True)
    assert np.allclose(n, [[0.6, 0.8], [0, 0], [7 / np.sqrt(113), 8 / np.sqrt(113)], [0, 0]], atol=1e-15)      # a zero vector stays zero
    rng = np.random.default_rng(2)
    B, S, H = 3, 6, 8
    x = rng.standard_normal((B, S, H)).astype(F32)
    plens = [6, 3, 1]
    mask = np.array([[1] * k + [0] * (S - k) for k in plens], np.uint32)
    packed = np.concatenate([x[b, :k] for b, k in enumerate(plens)])
    assert np.abs(R.pool_packed(packed, plens, R.POOL_MEAN, False) - O.mean_pool(x, mask)).max() < 1e-6
    assert np.abs(R.pool_padded(x, mask, R.POOL_MEAN, False) - O.mean_pool(x, mask)).max() < 1e-6
    assert np.abs(R.pool_padded(x, mask, R.POOL_MAX, True) - O.l2_normalize(O.max_pool(x, mask))).max() < 1e-6
    assert np.abs(R.pool_padded(x, mask, R.POOL_LAST, False) - O.last_token_pool(x, mask)).max() == 0


def test_head_references_by_hand():
    assert R.small_linear([[1, 2, 9], [3, 4, 9]], [[1, 1], [2, -1]], [10, 20], 2).tolist() == [[13, 20], [17, 22]]
    assert R.small_linear([[1, 2]], [[3, 4]], None, 2).tolist() == [[11]]
    p = R.row_softmax([[0, np.log(3.0)], [100, -100], [5, 5]], False)
    assert np.allclose(p, [[0.25, 0.75], [1, 0], [0.5, 0.5]], atol=1e-15)
    assert np.allclose(R.row_softmax([[0, np.log(3.0), -100]], True), [[0.5, 0.75, 0]], atol=1e-15)
