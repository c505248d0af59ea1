"""GGUF host side for Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q5_K (no GPU): kjarni_gguf_tensor_f32 bit-equal to numpy written from the
formats, block geometry through truncated files, and the refusals that name the tensor and the type."""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from tests import gguf_fixture as G
from tests import gguf_types_fixture as T

L = kjarni_amd.lib()
MD = {"general.architecture": "qwen2"}


def _tensor(path, name):
    n = C.c_size_t()
    shape = (C.c_int64 * 2)()
    nd = C.c_int32()
    rc = L.kjarni_gguf_tensor_f32(path.encode(), name.encode(), None, 0, C.byref(n), shape, C.byref(nd))
    if rc != 0:
        m = L.kjarni_last_error_message()
        return rc, m.decode() if m else ""
    out = np.empty(n.value, np.float32)
    rc = L.kjarni_gguf_tensor_f32(path.encode(), name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n), shape,
                                  C.byref(nd))
    assert rc == 0
    return 0, out.reshape(shape[0], shape[1])


def test_fixture_blocks_cover_every_code():
    rng = np.random.default_rng(0)
    for t in T.NEW_TYPES.values():
        k = 512
        b = T.random_blocks(t, 64, k, rng)
        w = T.dequantize(t, b, 64, k)
        assert np.isfinite(w).all() and 0.01 < w.std() < 0.04, (t, w.std())
    b = T.random_blocks(T.Q5_K, 64, 512, rng).reshape(-1, 176)
    sc, m = G._scale_min_k4(b[:, 4:16])
    assert set(np.unique(sc)) == set(range(64)) and set(np.unique(m)) == set(range(64))
    # pinned values, from the table of the formats
    blk = np.zeros(22, np.uint8)
    blk[0:2] = np.array([0.5], np.float16).view(np.uint8)
    blk[2:6] = np.array([1 | (1 << 17)], "<u4").view(np.uint8)   # fifth bit of elements 0 and 17
    blk[6] = 0x93                                                # element 0: nibble 3, element 16: nibble 9
    w = T.dequantize(T.Q5_0, blk, 1, 32)[0]
    assert w[0] == (3 + 16 - 16) * 0.5 and w[16] == (9 - 16) * 0.5 and w[17] == 0.0 and w[1] == -8.0
    blk = np.zeros(20, np.uint8)
    blk[0:2] = np.array([0.25], np.float16).view(np.uint8)
    blk[2:4] = np.array([-1.0], np.float16).view(np.uint8)
    blk[4 + 15] = 0xF0                                           # element 31: nibble 15
    w = T.dequantize(T.Q4_1, blk, 1, 32)[0]
    assert w[31] == 15 * 0.25 - 1.0 and w[15] == -1.0


@pytest.mark.parametrize("name", list(T.NEW_TYPES))
def test_tensor_f32_bit_exact(tmp_path, name):
    t = T.NEW_TYPES[name]
    rows, cols = 9, 768
    blocks = T.random_blocks(t, rows, cols, np.random.default_rng(t))
    p = G.write_gguf(str(tmp_path / "one.gguf"), MD, [("blk.0.attn_v.weight", t, (cols, rows), blocks)])
    rc, got = _tensor(p, "model.layers.0.self_attn.v_proj.weight")
    assert rc == 0, got
    ref = T.dequantize(t, blocks, rows, cols)
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", list(T.NEW_TYPES))
def test_block_geometry_through_truncation(tmp_path, name):
    t = T.NEW_TYPES[name]
    rows, cols = 2, 256
    blocks = T.random_blocks(t, rows, cols, np.random.default_rng(1))
    assert blocks.shape[1] == cols // T.BLOCK[t][0] * T.BLOCK[t][1]
    full = open(G.write_gguf(str(tmp_path / "ok.gguf"), MD, [("blk.0.attn_v.weight", t, (cols, rows), blocks)]), "rb").read()
    data = blocks.nbytes
    pad = (-data) % 32
    p = str(tmp_path / "cut.gguf")
    with open(p, "wb") as f:   # the last block is one byte short
        f.write(full[:len(full) - pad - 1])
    rc, msg = _tensor(p, "model.layers.0.self_attn.v_proj.weight")
    assert rc != 0 and "GGUF" in msg, msg
    with open(p, "wb") as f:   # every block present (padding dropped): loads
        f.write(full[:len(full) - pad])
    assert _tensor(p, "model.layers.0.self_attn.v_proj.weight")[0] == 0


@pytest.mark.parametrize("t", [12, 13], ids=["Q4_K", "Q5_K"])
def test_k_quant_at_224_columns_is_refused(tmp_path, t):
    raw = np.zeros((4, 176 if t == 13 else 144), np.uint8)
    p = G.write_gguf(str(tmp_path / "w.gguf"), MD, [("blk.0.attn_q.weight", t, (224, 4), raw)])
    rc, msg = _tensor(p, "model.layers.0.self_attn.q_proj.weight")
    assert rc != 0 and "blk.0.attn_q.weight" in msg and ("Q5_K" if t == 13 else "Q4_K") in msg and "224" in msg


def test_still_unsupported_type_is_named(tmp_path):
    raw = np.zeros((4, 110), np.uint8)   # Q3_K: 110 bytes per 256
    p = G.write_gguf(str(tmp_path / "q3.gguf"), MD, [("blk.0.attn_q.weight", 11, (256, 4), raw)])
    rc, msg = _tensor(p, "model.layers.0.self_attn.q_proj.weight")
    assert rc != 0 and "Q3_K" in msg and "(11)" in msg and "blk.0.attn_q.weight" in msg
    assert "Q5_K" in msg and "Q5_0" in msg   # the list of what is supported names the new types
