"""FP8 (e4m3fn) checkpoints, host side (no GPU): the new symbols' declarations and NULL behaviour, kjarni_fp8_tensor_f32 -- the
loader's own reading and dequantization -- bit for bit against tests/fp8_fixture.py's f32 twin, and every load refusal with the
tensor named in the message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fp8_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "model.layers.0.mlp.up_proj.weight"
NULL_POINTER = 1  # KJARNI_ERROR_NULL_POINTER


def _lib():
    import kjarni_amd
    return kjarni_amd.lib()


def _tensor(path, name=NAME):
    """(rc, array or None, last error)"""
    import kjarni_amd._ffi as ffi
    L = _lib()
    n, nd = C.c_size_t(0), C.c_int32(0)
    shape = (C.c_int64 * 2)()
    rc = L.kjarni_fp8_tensor_f32(path.encode(), name.encode(), None, 0, C.byref(n), shape, C.byref(nd))
    if rc != 0:
        return rc, None, ffi.last_error()
    assert nd.value == 2 and shape[0] * shape[1] == n.value
    out = np.empty((shape[0], shape[1]), np.float32)
    rc = L.kjarni_fp8_tensor_f32(path.encode(), name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n), shape,
                                 C.byref(nd))
    assert rc == 0
    return 0, out, ""


def _one(tmp, tag, kind, n=200, k=384, seed=0, cfg=None, **kw):
    """A directory with one FP8 matrix; returns (path, codes, scale, twin)."""
    rng = np.random.default_rng(seed)
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    if kw.get("scale_dtype") == "BF16":
        scale = F.bf16_exact(scale)
    shards = kw.pop("shards", 1)
    extra = kw.pop("extra", {})
    t = F.matrix_entries(NAME, codes, scale, kind, **kw)
    t.update(extra)
    if shards > 1:  # more tensors, so that the weight and its scale are in different files
        t["model.norm.weight"] = F.entry(np.ones(k, np.float32))
    path = F.write_dir(str(tmp / tag), cfg, t, shards)
    return path, codes, scale, F.dequantize(codes, scale, kind)


def test_table_and_encoder():
    t = F.TABLE
    assert np.isnan(t[0x7F]) and np.isnan(t[0xFF]) and np.nanmax(t) == 448.0 and np.nanmin(t) == -448.0
    assert t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6 and t[0x38] == 1.0 and t[0x7E] == 448.0 and t[0x80] == 0.0 and np.signbit(t[0x80])
    torch = pytest.importorskip("torch")
    if hasattr(torch, "float8_e4m3fn"):
        ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
        assert np.array_equal(ref.view(np.uint32)[F.FINITE_CODES], t.view(np.uint32)[F.FINITE_CODES])
    assert F.FINITE_CODES.size == 254
    # every finite code encodes to itself (-0 included); values between two codes go to the nearest, ties to the even code
    assert np.array_equal(F.encode(t[F.FINITE_CODES]), F.FINITE_CODES)
    assert F.encode(np.array([1000.0, -1000.0, 1.0625, 1.1875, 1.07])).tolist() == [0x7E, 0xFE, 0x38, 0x3A, 0x39]


def test_declarations_and_ffi_mirror():
    import kjarni_amd._ffi as ffi
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    for name, arity in (("kjarni_fp8_tensor_f32", 7), ("kjarni_hip_op_linear_fp8", 10)):
        m = re.search(r"KjarniErrorCode\s+" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        restype, argtypes = ffi.SIGNATURES[name]
        fn = getattr(_lib(), name)
        assert len(fn.argtypes) == arity and fn.restype is C.c_int32
        assert len(argtypes) == arity and restype is C.c_int32
    m = re.search(r"#define\s+KJARNI_HIP_WEIGHT_TYPE_F8_E4M3\s+(\d+)", header)
    from kjarni_amd import decoder
    assert m and int(m.group(1)) == decoder.WEIGHT_TYPE_F8_E4M3 and int(m.group(1)) < 32
    assert int(m.group(1)) not in (0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 30)      # the GGML types this project reads
    assert "F8_E4M3" in header[header.index("kjarni_hip_decoder_load") - 3000:header.index("kjarni_hip_decoder_load")]


def test_null_arguments():
    L = _lib()
    n = C.c_size_t(7)
    f = (C.c_float * 4)()
    assert L.kjarni_fp8_tensor_f32(None, b"x", None, 0, C.byref(n), None, None) == NULL_POINTER
    assert L.kjarni_fp8_tensor_f32(b"/nonexistent", None, None, 0, C.byref(n), None, None) == NULL_POINTER
    assert L.kjarni_fp8_tensor_f32(b"/nonexistent", b"x", None, 0, None, None, None) == NULL_POINTER
    assert L.kjarni_fp8_tensor_f32(b"/nonexistent", b"x", None, 4, C.byref(n), None, None) == NULL_POINTER
    rc = L.kjarni_fp8_tensor_f32(b"/nonexistent-dir", b"x", f, 4, C.byref(n), None, None)      # a load error, not a crash
    assert rc not in (0, NULL_POINTER) and n.value == 0
    u8 = (C.c_uint8 * 16)()
    for args in ((None, 1, u8, f, 1, 1, 1, 16, f), (f, 1, None, f, 1, 1, 1, 16, f), (f, 1, u8, None, 1, 1, 1, 16, f),
                 (f, 1, u8, f, 1, 1, 1, 16, None)):
        assert L.kjarni_hip_op_linear_fp8(0, *args) == NULL_POINTER


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("scale_dtype", ["F32", "BF16"])
def test_tensor_bit_for_bit(tmp_path, kind, scale_dtype):
    path, codes, scale, twin = _one(tmp_path, "m", kind, scale_dtype=scale_dtype, seed=3)
    assert codes.shape == (200, 384) and (kind != "block" or scale.shape == (2, 3))     # n = 200: the last block row is partial
    rc, got, err = _tensor(path)
    assert rc == 0, err
    assert np.array_equal(got.view(np.uint32), twin.view(np.uint32))
    assert len(np.unique(codes)) > 100 and np.unique(scale).size > scale.size // 2      # (the fixture: many codes, scales that differ)


def test_scale_names_shapes_and_shards(tmp_path):
    # both names mean w = decode(code) * scale; [n] and [n, 1]; an F16 scale; a sharded directory
    for tag, kind, kw in (("inv", "channel", dict(scale_name="weight_scale_inv")), ("plain", "block", dict(scale_name="weight_scale")),
                          ("flat", "channel", dict(flat_channel=True)), ("shard", "block", dict(shards=3)),
                          ("shard2", "tensor", dict(shards=2))):
        path, codes, scale, twin = _one(tmp_path, tag, kind, seed=5, **kw)
        rc, got, err = _tensor(path)
        assert rc == 0, (tag, err)
        assert np.array_equal(got.view(np.uint32), twin.view(np.uint32)), tag
    assert len([f for f in os.listdir(str(tmp_path / "shard")) if f.endswith(".safetensors")]) == 3
    rng = np.random.default_rng(1)
    codes, scale = F.quantize(rng.standard_normal((64, 128)).astype(np.float32), "channel", rng)
    scale = scale.astype(np.float16).astype(np.float32)
    path = F.write_dir(str(tmp_path / "f16"), None, F.matrix_entries(NAME, codes, scale, "channel", scale_dtype="F16"))
    rc, got, err = _tensor(path)
    assert rc == 0, err
    assert np.array_equal(got.view(np.uint32), F.dequantize(codes, scale, "channel").view(np.uint32))


def _refused(tmp, tag, kind="channel", **kw):
    path = _one(tmp, tag, kind, **kw)[0]
    rc, got, err = _tensor(path)
    assert rc != 0 and got is None and NAME in err, (tag, rc, err)
    return err


def test_refusals_name_the_tensor(tmp_path):
    s = NAME[:-len("weight")]
    # a missing scale
    rng = np.random.default_rng(0)
    codes, scale = F.quantize(rng.standard_normal((32, 64)).astype(np.float32), "tensor", rng)
    path = F.write_dir(str(tmp_path / "noscale"), None, {NAME: F.entry(codes)})
    rc, _, err = _tensor(path)
    assert rc != 0 and NAME in err and "no scale" in err and "weight_scale_inv" in err
    # both scale names
    err = _refused(tmp_path, "both", extra={s + "weight_scale_inv": F.entry(np.ones((200, 1), np.float32))})
    assert "both" in err and s + "weight_scale_inv" in err and s + "weight_scale" in err
    # a scale shape that fits no kind (and says what was found)
    for i, shape in enumerate(((199, 1), (2, 2), (3, 3), (2, 3, 1), (200, 384))):
        t = {NAME: F.entry(np.zeros((200, 384), np.uint8)), s + "weight_scale": F.entry(np.ones(shape, np.float32))}
        rc, _, err = _tensor(F.write_dir(str(tmp_path / f"shape{i}"), None, t))
        assert rc != 0 and NAME in err and str(list(shape)) in err, err
    # block scales need k % 128 == 0: [2, 3] beside k = 400 fits nothing
    t = {NAME: F.entry(np.zeros((200, 400), np.uint8)), s + "weight_scale_inv": F.entry(np.ones((2, 3), np.float32))}
    rc, _, err = _tensor(F.write_dir(str(tmp_path / "k400"), None, t))
    assert rc != 0 and NAME in err
    # k % 16
    t = {NAME: F.entry(np.zeros((8, 24), np.uint8)), s + "weight_scale": F.entry(np.ones(1, np.float32))}
    rc, _, err = _tensor(F.write_dir(str(tmp_path / "k24"), None, t))
    assert rc != 0 and NAME in err and "16" in err
    # a block size other than 128, another fmt
    err = _refused(tmp_path, "bs64", "block", cfg={"quantization_config": {"fmt": "e4m3", "weight_block_size": [64, 64]}})
    assert "[64, 64]" in err and "128" in err
    err = _refused(tmp_path, "e5m2", cfg={"quantization_config": {"fmt": "e5m2"}})
    assert "e5m2" in err and "e4m3" in err
    assert _tensor(_one(tmp_path, "fmt-ok", "block", cfg={"quantization_config": {"fmt": "e4m3", "weight_block_size": [128, 128]}})[0])[0] == 0
    # a NaN code, either sign
    for code in (0x7F, 0xFF):
        codes = np.zeros((16, 32), np.uint8)
        codes[5, 7] = code
        t = {NAME: F.entry(codes), s + "weight_scale": F.entry(np.ones(1, np.float32))}
        rc, _, err = _tensor(F.write_dir(str(tmp_path / f"nan{code}"), None, t))
        assert rc != 0 and NAME in err and "NaN" in err and f"0x{code:02X}" in err and "row 5" in err
    # a tensor that is not there, and one that is not FP8
    t = {NAME: F.entry(np.ones((4, 16), np.float32))}
    path = F.write_dir(str(tmp_path / "f32"), None, t)
    rc, _, err = _tensor(path)
    assert rc != 0 and NAME in err and "F32" in err
    rc, _, err = _tensor(path, "nothing.weight")
    assert rc != 0 and "nothing.weight" in err
