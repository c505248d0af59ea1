"""Qwen3-MoE without a GPU: the three new entry points are declared, exported and bound with their arity and answer NULL as
declared; the loader checks a qwen3_moe directory on the host, before it asks for a device, and names what it refuses; the
sparse-layer rule against a table; the two ops refuse bad arguments before any GPU work, outputs untouched; the float64
reference (tests/moe_ref64.py) against the dense reference in the two cases where they must agree; the fixture's seeds clear
their margins; the registry knows the two names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, ops
from kjarni_amd._ffi import KjarniError as E
from tests import moe_fixture as F
from tests.moe_ref64 import MoeRef64, moe_ffn64, route64, router_margins
from tests.qwen3_ref64 import Qwen3Ref64, assert_margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()
SYMBOLS = {"kjarni_hip_op_moe_route": 8, "kjarni_hip_op_moe_ffn": 26, "kjarni_hip_decoder_moe_routing": 6}


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


def _ffn_args(f, i, used, tiles):
    v = C.cast(f, C.c_void_p)
    return [0, f, 64, 1, None, 1e-6, v, v, v, v, 0, 64, 8, 2, 32, 0, f, 64, 0, f, 64, 0, i, f, C.byref(used), C.byref(tiles)]


def test_null_pointers():
    f, i = (C.c_float * 64)(), (C.c_int32 * 16)()
    args = [0, f, 1, 8, 2, 0, i, f]
    for at in (1, 6, 7):                                                 # logits, ids_out, weights_out
        bad = list(args)
        bad[at] = None
        assert L.kjarni_hip_op_moe_route(*bad) == E.NULL_POINTER
    used, tiles = C.c_int32(-5), C.c_int32(-5)
    for at in (1, 6, 7, 8, 9, 19, 22, 23, 24, 25):                      # x, router, gate, up, down, y, ids, weights, route_used, tiles_used
        bad = _ffn_args(f, i, used, tiles)
        bad[at] = None
        assert L.kjarni_hip_op_moe_ffn(*bad) == E.NULL_POINTER
    n = C.c_int32(-5)
    assert L.kjarni_hip_decoder_moe_routing(None, 0, 0, C.byref(n), None, None) == E.NULL_POINTER
    assert (used.value, tiles.value, n.value) == (-5, -5, -5) and not any(f) and not any(i)


# ---- the ops' argument checks come before any GPU work ------------------------------------------------------------------------------

@pytest.mark.parametrize("E_,k,rows,word", [(1, 1, 1, "E"), (257, 1, 1, "E"), (8, 0, 1, "k"), (8, 9, 1, "k"), (4, 5, 1, "k"), (8, 2, 0, "rows")])
def test_moe_route_refuses_before_any_gpu_work(E_, k, rows, word):
    logits = np.zeros((max(rows, 1), E_), np.float32)
    ids, w = np.full((max(rows, 1), 8), -7, np.int32), np.full((max(rows, 1), 8), 7.0, np.float32)
    rc = L.kjarni_hip_op_moe_route(0, logits.ctypes.data_as(_ffi._f32p), rows, E_, k, 0, ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                   w.ctypes.data_as(_ffi._f32p))
    msg = (L.kjarni_last_error_message() or b"").decode()
    assert rc == E.INVALID_CONFIG and word in msg, (rc, msg)
    assert (ids == -7).all() and (w == 7.0).all()


def _ffn_call(hidden=64, Im=32, E_=8, k=2, rows=2, ldx=None, ldy=None, route=0, residual=True):
    x = np.zeros((max(rows, 1), ldx or hidden), np.float32)
    y = np.full((max(rows, 1), ldy or hidden), 7.0, np.float32)
    rt = np.zeros((E_, hidden), np.float32)
    g, d = np.zeros((E_, Im, hidden), np.float32), np.zeros((E_, hidden, Im), np.float32)
    ids, w = np.full((max(rows, 1), 8), -7, np.int32), np.full((max(rows, 1), 8), 7.0, np.float32)
    used, tiles = C.c_int32(-5), C.c_int32(-5)
    p, v = (lambda a: a.ctypes.data_as(_ffi._f32p)), (lambda a: a.ctypes.data_as(C.c_void_p))
    rc = L.kjarni_hip_op_moe_ffn(0, p(x), x.shape[1], rows, None, 1e-6, v(rt), v(g), v(g), v(d), 0, hidden, E_, k, Im, 0, None, 0,
                                 1 if residual else 0, p(y), y.shape[1], route, ids.ctypes.data_as(C.POINTER(C.c_int32)), p(w), C.byref(used),
                                 C.byref(tiles))
    untouched = (y == 7.0).all() and (ids == -7).all() and (w == 7.0).all() and used.value == -5 and tiles.value == -5
    return rc, (L.kjarni_last_error_message() or b"").decode(), untouched


@pytest.mark.parametrize("kw,word", [(dict(E_=1), "E"), (dict(k=0), "k"), (dict(k=3, E_=2), "k"), (dict(Im=48), "Im"), (dict(hidden=72), "hidden"),
                                      (dict(rows=0), "rows"), (dict(rows=4097), "rows"), (dict(ldx=32), "ldx"), (dict(ldy=66), "ldy"),
                                      (dict(route=3), "route"), (dict(residual=False), "residual"), (dict(k=8, Im=4096, E_=8), "k * Im")])
def test_moe_ffn_refuses_before_any_gpu_work(kw, word):
    rc, msg, untouched = _ffn_call(**kw)
    assert rc == E.INVALID_CONFIG and word in msg, (kw, rc, msg)
    assert untouched


def test_ops_wrappers_check_shapes():
    z = np.zeros
    with pytest.raises(ValueError):
        ops.moe_route(z(8, np.float32), 2)
    with pytest.raises(ValueError):
        ops.moe_ffn(z((2, 64)), z((8, 64)), z((8, 32, 64)), z((8, 32, 64)), z((8, 32, 64)), 2, z((2, 64)), r_is_y=True)   # down is [E, hidden, Im]


# ---- the loader: a qwen3_moe directory is checked on the host, before a device is asked for ------------------------------------------

def _load(path):
    h = C.c_void_p()
    rc = L.kjarni_hip_decoder_load(path.encode(), 0, 0, 0, C.byref(h))
    msg = (L.kjarni_last_error_message() or b"").decode() if rc else ""
    if rc == 0:
        L.kjarni_hip_decoder_free(h)
    return rc, msg


def _accepted(rc, msg):
    """The directory passed every host check: it loaded, or (no GPU here) the only complaint is the missing device."""
    return rc == E.OK or (rc == E.GPU_UNAVAILABLE and "model_type" not in msg and "tensor" not in msg)


def test_a_qwen3_moe_directory_passes_the_host_checks(tmp_path):
    for name, geo in F.GEOMETRIES.items():
        if name == "MOE_WIDE":
            continue
        cfg, t = F.moe_model(str(tmp_path / name), geo)
        rc, msg = _load(str(tmp_path / name))
        assert _accepted(rc, msg), (name, rc, msg)      # the parent commit: "unsupported decoder model_type 'qwen3_moe'"
    # the config fields reach the parsed config (config_json carries them as they are)
    assert cfg["num_experts"] == 8 and cfg["mlp_only_layers"] == [0]


def _refused(tmp_path, tag, cfg_over=None, drop=(), replace=None, extra=None):
    cfg = dict(F.MOE_SMALL)
    cfg.update(cfg_over or {})
    t = F.moe_tensors(dict(F.MOE_SMALL), F.MODEL_SEED)
    t = {k: v for k, v in t.items() if k not in drop}
    t.update(replace or {})
    t.update(extra or {})
    rc, msg = _load(F.write_dir(str(tmp_path / tag), cfg, t))
    assert rc == E.LOAD_FAILED, (tag, rc, msg)
    return msg


def test_loader_refusals_name_what_was_found(tmp_path):
    for val in (1, 257):
        msg = _refused(tmp_path, f"E{val}", {"num_experts": val})
        assert "num_experts" in msg and str(val) in msg, msg
    for val, e in ((0, 8), (9, 16), (3, 2)):
        msg = _refused(tmp_path, f"k{val}", {"num_experts_per_tok": val, "num_experts": e})
        assert "num_experts_per_tok" in msg and str(val) in msg, msg
    msg = _refused(tmp_path, "im48", {"moe_intermediate_size": 48})
    assert "moe_intermediate_size" in msg and "48" in msg and "32" in msg, msg
    name = "model.layers.1.mlp.experts.5.up_proj.weight"
    assert name in _refused(tmp_path, "missing", drop=(name,))
    msg = _refused(tmp_path, "shape", replace={name: np.zeros((32, 32), np.float32)})
    assert name in msg and "[32, 32]" in msg and "[32, 64]" in msg, msg
    router = "model.layers.0.mlp.gate.weight"
    assert router in _refused(tmp_path, "norouter", drop=(router,))
    msg = _refused(tmp_path, "routershape", replace={router: np.zeros((7, 64), np.float32)})
    assert router in msg and "[7, 64]" in msg, msg
    dense = "model.layers.0.mlp.gate_proj.weight"
    msg = _refused(tmp_path, "dense", extra={dense: np.zeros((96, 64), np.float32)})
    assert dense in msg and "sparse layer 0" in msg, msg
    msg = _refused(tmp_path, "quantcfg", {"quantization_config": {"fmt": "e4m3"}})
    assert "out of scope" in msg and "FP8" in msg, msg
    msg = _refused(tmp_path, "f8", replace={name: np.zeros((32, 64), np.uint8)})      # (any dtype but the float ones names the tensor too)
    assert name in msg, msg


def test_fp8_expert_tensor_is_refused_as_out_of_scope(tmp_path):
    import json
    import torch
    from safetensors.torch import save_file
    cfg = dict(F.MOE_SMALL)
    t = F.moe_tensors(cfg, F.MODEL_SEED)
    name = "model.layers.0.mlp.experts.0.gate_proj.weight"
    d = tmp_path / "fp8"
    d.mkdir()
    json.dump(cfg, open(d / "config.json", "w"))
    save_file({k: (torch.from_numpy(v).to(torch.float8_e4m3fn) if k == name else torch.from_numpy(v)) for k, v in t.items()},
              str(d / "model.safetensors"))
    rc, msg = _load(str(d))
    assert rc == E.LOAD_FAILED and name in msg and "F8_E4M3" in msg and "out of scope" in msg, (rc, msg)


def test_gguf_qwen3moe_is_refused_as_out_of_scope(tmp_path):
    from tests import gguf_fixture as G
    md = {"general.architecture": "qwen3moe", "general.name": "fixture", "qwen3moe.embedding_length": 256, "qwen3moe.block_count": 1}
    emb = G.random_blocks(8, 50, 256, np.random.default_rng(0))
    p = G.write_gguf(str(tmp_path / "moe.gguf"), md, [("token_embd.weight", 8, (256, 50), emb)])
    out = C.c_void_p()
    rc = L.kjarni_gguf_config_json(p.encode(), C.byref(out))
    msg = (L.kjarni_last_error_message() or b"").decode()
    assert rc != 0 and "qwen3moe" in msg and "out of scope" in msg and "GGUF" in msg, msg


# (decoder_sparse_step, mlp_only_layers) -> the sparse layers of a 4-layer model
SPARSE_TABLE = [(1, [], [0, 1, 2, 3]), (2, [], [1, 3]), (3, [], [2]), (1, [0], [1, 2, 3]), (2, [1], [3]), (1, [0, 1, 2, 3], []), (5, [], []),
                (4, [2], [3])]


@pytest.mark.parametrize("step,only,sparse", SPARSE_TABLE)
def test_sparse_layer_rule(tmp_path, step, only, sparse):
    geo = dict(F.MOE_SMALL, num_hidden_layers=4, decoder_sparse_step=step, mlp_only_layers=only)
    t = F.moe_tensors(geo, 0)
    assert [i for i in range(4) if f"model.layers.{i}.mlp.gate.weight" in t] == sparse          # the fixture restates the rule ...
    assert [i for i in range(4) if MoeRef64(t, geo).sparse(i)] == sparse                          # ... as does the reference ...
    rc, msg = _load(F.write_dir(str(tmp_path / "ok"), geo, t))
    assert _accepted(rc, msg), (rc, msg)                                                          # ... and the loader agrees:
    for i in range(4):   # each layer laid out as the other kind is refused, naming a tensor of that layer
        bad = {k: v for k, v in t.items() if not k.startswith(f"model.layers.{i}.mlp.")}
        other = F.moe_tensors(dict(geo, mlp_only_layers=[i]) if i in sparse else dict(geo, decoder_sparse_step=1, mlp_only_layers=[]), 0)
        bad.update({k: v for k, v in other.items() if k.startswith(f"model.layers.{i}.mlp.")})
        rc, msg = _load(F.write_dir(str(tmp_path / f"bad{i}"), geo, bad))
        assert rc == E.LOAD_FAILED and f"model.layers.{i}.mlp." in msg, (i, rc, msg)


# ---- the float64 reference -------------------------------------------------------------------------------------------------------------

def test_one_expert_is_the_dense_layer():
    """E = k = 1: softmax over one expert is 1, so the sparse layer is the dense SwiGLU on the same matrices."""
    geo = dict(F.MOE_SMALL, num_experts=1, num_experts_per_tok=1)
    t = F.moe_tensors(geo, 3)
    dense_geo = dict(geo, model_type="qwen3", intermediate_size=geo["moe_intermediate_size"])
    dense = {k: v for k, v in t.items() if ".mlp." not in k}
    for i in range(geo["num_hidden_layers"]):
        for nm in ("gate_proj", "up_proj", "down_proj"):
            dense[f"model.layers.{i}.mlp.{nm}.weight"] = t[f"model.layers.{i}.mlp.experts.0.{nm}.weight"]
    ids = F.seeded_prompt(1, 300, 11)
    a, b = MoeRef64(t, geo), Qwen3Ref64(dense, dense_geo)
    ha, hb = a.forward(ids, a.new_cache()), b.forward(ids, b.new_cache())
    assert np.abs(ha - hb).max() <= 1e-13 * np.abs(hb).max()
    for norm in (False, True):
        assert np.array_equal(route64(np.array([[0.3]]), 1, norm)[1], [[1.0]])


def test_uniform_router_with_norm_topk_is_the_mean_of_the_first_k_experts():
    rng = np.random.default_rng(0)
    H, Im, E_, k = 16, 8, 6, 3
    x = rng.standard_normal((5, H))
    gate, up, down = rng.standard_normal((E_, Im, H)), rng.standard_normal((E_, Im, H)), rng.standard_normal((E_, H, Im))
    out, r, ids, w = moe_ffn64(x, np.zeros((E_, H)), gate, up, down, k, True)
    assert (ids == np.arange(k)).all() and np.allclose(w, 1.0 / k, rtol=0, atol=1e-16)      # ties: the lower index first
    g = np.einsum("eih,rh->rei", gate[:k], x)
    want = np.einsum("ehi,rei->rh", down[:k], g / (1 + np.exp(-g)) * np.einsum("eih,rh->rei", up[:k], x)) / k
    assert np.abs(out - want).max() <= 1e-12 * np.abs(want).max()
    _, _, _, w2 = moe_ffn64(x, np.zeros((E_, H)), gate, up, down, k, False)
    assert np.allclose(w2, 1.0 / E_, rtol=0, atol=1e-16)


def test_route64_ties_and_extremes():
    r = np.array([[1.0, 3.0, 3.0, 0.0, 3.0], [60.0, -60.0, -60.0, 0.0, -60.0]])
    ids, w = route64(r, 3, False)
    assert ids.tolist() == [[1, 2, 4], [0, 3, 1]]
    assert w[1, 2] > 0.0 and w[1, 0] >= 1.0 - 1e-15               # float64 keeps exp(-120)
    assert router_margins(r[:1], 3).tolist() == [False]           # (3.0, 3.0, 3.0 | 1.0): the set is clear, the order a tie
    assert router_margins(np.array([[5.0, 1.0, 4.9995, 0.0]]), 2).tolist() == [False]      # the set is clear, the order inside is not
    with pytest.raises(AssertionError):
        router_margins(np.array([[5.0, 1.0, 1.0005, 0.0]]), 2)


# ---- the seeds of the GPU tests ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,bf16", sorted(F.GREEDY_PROMPT_SEED))
def test_seeds_clear_their_margins(name, bf16):
    geo = F.GEOMETRIES[name]
    t = F.moe_tensors(geo, F.MODEL_SEED, bf16=bf16)
    ref = MoeRef64(t, geo)
    ids, gaps, tops = ref.greedy(F.seeded_prompt(F.GREEDY_PROMPT_SEED[(name, bf16)], geo["vocab_size"], 9), 12)
    assert_margins(gaps, tops, name)
    ref.assert_router_margins(name)
    assert geo["eos_token_id"] not in ids
    ref = MoeRef64(t, geo)
    ref.forward(F.seeded_prompt(F.LONG_PROMPT_SEED[(name, bf16)], geo["vocab_size"], 40), ref.new_cache())
    ref.assert_router_margins(name + " long")
    n_sparse = sum(ref.sparse(i) for i in range(ref.L))
    assert sorted(ref.routing) == [i for i in range(ref.L) if ref.sparse(i)] and n_sparse == (1 if name == "MOE_MIXED" else 2)


def test_lane_and_lookup_seeds_clear_their_margins():
    from tests import qwen3_fixture as Q3
    geo = F.MOE_WIDE
    t = F.moe_tensors(geo, F.MODEL_SEED)
    cases = [(F.seeded_prompt(seed, geo["vocab_size"], n), 8) for n, seed in F.LANE_PROMPTS]
    for prompt, n in cases + [(Q3.lookup_prompt(F.LOOKUP_PROMPT_SEED, geo["vocab_size"]), 12)]:
        ref = MoeRef64(t, geo)
        ids, gaps, tops = ref.greedy(prompt, n)
        assert_margins(gaps, tops, f"prompt of {len(prompt)}")
        ref.assert_router_margins(f"prompt of {len(prompt)}")
        assert geo["eos_token_id"] not in ids


# ---- registry ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cli,repo", [("qwen3-30b-a3b", "Qwen/Qwen3-30B-A3B"), ("qwen3-30b-a3b-instruct-2507", "Qwen/Qwen3-30B-A3B-Instruct-2507")])
def test_registry_resolves_the_moe_names(cli, repo, tmp_path):
    from kjarni_amd.chat import Chat
    for name in (cli, repo, repo.lower(), cli.upper()):
        with pytest.raises(_ffi.KjarniException) as e:     # known, ChatML family, nothing on disk
            Chat(name, cache_dir=str(tmp_path / "empty"))
        assert e.value.code == E.MODEL_NOT_FOUND and f"model '{cli}' not downloaded" in str(e.value), str(e.value)
