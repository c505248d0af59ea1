"""FP8 Qwen3-MoE without a GPU: kjarni_hip_op_moe_ffn_fp8's declaration, arity, NULL answers and refusals (outputs untouched); the
loader's host checks on an FP8 qwen3_moe directory and each new refusal.  Also the fixture of both test files: tests/moe_fixture.py's
tensors with every `*_proj.weight` quantized by tests/fp8_fixture.py (the float64 reference runs on the dequantized tensors)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from tests import fp8_fixture as Q
from tests import moe_fixture as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
NAME, ARITY = "kjarni_hip_op_moe_ffn_fp8", 28
# hidden, Im, intermediate_size 256: every matrix but Q (128 x 256: [1, 2]) has at least two blocks; layer 0 dense, layer 1 sparse
MOE_F8 = F._geometry(256, 2, 4, 2, 32, 256, 300, 256, E=8, k=2, Im=256, norm_topk=True, mlp_only_layers=[0])
# seeds chosen on the CPU with the reference alone (tools/moe_seed_search.py's rule: router and vocabulary margins above 100 bars)
GREEDY_PROMPT_SEED = {"block": 18, "channel": 1}    # 9-token prompts, 12 greedy tokens
LONG_PROMPT_SEED = {"block": 19, "channel": 152}    # 130-token prompts (and their first 24 tokens)
LANE_PROMPT_SEEDS = (100, 101, 103, 112, 114, 120, 122, 123, 128, 129, 138, 139, 141, 143, 149, 154)     # block: prompt i has 3 + i tokens, 8 greedy tokens each

def fp8_moe_model(path, kind, edit=None, quant=None, **over):
    """Writes the directory; returns (config, dequantized HF tensors).  edit(name, codes, scale, kind) may return other entries."""
    cfg = dict(MOE_F8, **over)
    cfg["quantization_config"] = quant or dict({"quant_method": "fp8", "fmt": "e4m3"}, **({"weight_block_size": [128, 128]} if kind == "block" else {}))
    rng = np.random.default_rng(1005)
    st, hf = {}, {}
    for name, a in F.moe_tensors(cfg, 5).items():
        if not name.endswith("_proj.weight"):
            st[name], hf[name] = Q.entry(a), a
            continue
        codes, scale = Q.quantize(a, kind, rng)
        hf[name] = Q.dequantize(codes, scale, kind)
        st.update((edit and edit(name, codes, scale, kind)) or Q.matrix_entries(name, codes, scale, kind))
    Q.write_dir(path, cfg, st)
    return cfg, hf

def test_symbol_is_declared_exported_and_bound_with_its_arity():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    decl = re.search(r"\b" + NAME + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert decl, f"{NAME} is not declared in include/kjarni_hip.h"
    assert hasattr(L, NAME), f"{NAME} is not exported"
    restype, argtypes = _ffi.SIGNATURES[NAME]
    assert restype is C.c_int32 and len(argtypes) == ARITY == len([a for a in decl.group(1).split(",") if a.strip()])

def _call(hidden=128, Im=128, E_=4, k=2, rows=2, kind=2, ldx=None, ldy=None, grouped=0, residual=True, nan_code=False, null=None):
    x, y = np.zeros((max(rows, 1), ldx or hidden), np.float32), np.full((max(rows, 1), ldy or hidden), 7.0, np.float32)
    rt, sc = np.zeros((E_, hidden), np.float32), np.ones(E_ * max(hidden, Im), np.float32)
    g, d = np.zeros((E_, Im, hidden), np.uint8), np.zeros((E_, hidden, Im), np.uint8)
    d[-1, -1, -1] = 0xFF if nan_code else 0
    ids, w, tiles = np.full((max(rows, 1), 8), -7, np.int32), np.full((max(rows, 1), 8), 7.0, np.float32), C.c_int32(-5)
    p, v = (lambda a: a.ctypes.data_as(_ffi._f32p)), (lambda a: a.ctypes.data_as(C.c_void_p))
    args = [0, p(x), x.shape[1], rows, None, 1e-6, p(rt), v(g), p(sc), v(g), p(sc), v(d), p(sc), kind, hidden, E_, k, Im, 0, None, 0,
            1 if residual else 0, p(y), y.shape[1], grouped, ids.ctypes.data_as(C.POINTER(C.c_int32)), p(w), C.byref(tiles)]
    if null is not None:
        args[null] = None
    rc = getattr(L, NAME)(*args)
    untouched = (y == 7.0).all() and (ids == -7).all() and (w == 7.0).all() and tiles.value == -5
    return rc, (L.kjarni_last_error_message() or b"").decode(), untouched

NULLS = [(dict(null=at), None) for at in (1, 6, 7, 8, 9, 10, 11, 12, 22, 25, 26, 27)]     # x, router, six stack pointers, y, ids, weights, tiles

@pytest.mark.parametrize("kw,word", NULLS + [
    (dict(E_=1), "E"), (dict(k=0), "k"), (dict(k=3, E_=2), "k"), (dict(Im=48), "Im"), (dict(hidden=72), "hidden"), (dict(rows=0), "rows"),
    (dict(rows=4097), "rows"), (dict(ldx=32), "ldx"), (dict(ldy=130), "ldy"), (dict(grouped=2), "grouped"), (dict(residual=False), "residual"),
    (dict(kind=3), "kind"), (dict(kind=-1), "kind"), (dict(hidden=96), "multiple of 128"), (dict(Im=96), "multiple of 128"),
    (dict(nan_code=True), "NaN code")])
def test_null_and_refusals_before_any_gpu_work(kw, word):
    rc, msg, untouched = _call(**kw)
    assert untouched and (rc == E.NULL_POINTER if word is None else rc == E.INVALID_CONFIG and word in msg), (kw, rc, msg)

# ---- the loader ---------------------------------------------------------------------------------------------------------------------------

def _load(path):
    h = C.c_void_p()
    rc = L.kjarni_hip_decoder_load(path.encode(), 0, 0, 0, C.byref(h))
    msg = (L.kjarni_last_error_message() or b"").decode() if rc else ""
    if rc == 0:
        L.kjarni_hip_decoder_free(h)
    return rc, msg

@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("method", ["fp8", "compressed-tensors"])
def test_an_fp8_directory_passes_the_host_checks(tmp_path, kind, method):
    fp8_moe_model(str(tmp_path / "m"), kind, quant={"quant_method": method})
    rc, msg = _load(str(tmp_path / "m"))      # the parent commit: "... are out of scope"
    assert rc == E.OK or (rc == E.GPU_UNAVAILABLE and "model_type" not in msg and "tensor" not in msg), (rc, msg)

EXPERT = "model.layers.1.mlp.experts.5.up_proj.weight"
ME = Q.matrix_entries
BLOCKS96 = dict(moe_intermediate_size=96, num_experts_per_tok=1, intermediate_size=384)
EDITS = {   # one tensor wrong: left F32; per-tensor scales in a per-channel stack; two scale tensors; [ceil(n / 128), ceil(k / 128)] scales at Im 96
    "f32": (lambda n, c, s, k: {n: Q.entry(Q.dequantize(c, s, k))} if n == EXPERT else None, [EXPERT, "F32", "F8_E4M3"], {}),
    "kind": (lambda n, c, s, k: ME(n, c, s[:1], "tensor") if n == EXPERT else None, [EXPERT, "per tensor", "per channel"], {}),
    "two": (lambda n, c, s, k: dict(ME(n, c, s, k), **ME(n, c, s, k, scale_name="weight_scale_inv")) if n == EXPERT else None,
            [EXPERT, "weight_scale_inv", "exactly one"], {}),
    "blocks": (lambda n, c, s, k: {n: Q.entry(c), n + "_scale_inv": Q.entry(np.ones((-(-c.shape[0] // 128), -(-c.shape[1] // 128)), np.float32))},
               ["block scales", "moe_intermediate_size 96", "128", "weight"], BLOCKS96)}

@pytest.mark.parametrize("tag", sorted(EDITS))
def test_loader_refusals_name_the_tensor_and_what_was_found(tmp_path, tag):
    edit, words, over = EDITS[tag]
    fp8_moe_model(str(tmp_path / "m"), "channel", edit=edit, **over)
    rc, msg = _load(str(tmp_path / "m"))
    assert rc == E.LOAD_FAILED and all(w in msg for w in words), (rc, msg)
