"""Pins tests/llm_ref64.py (the float64 KV-cache reference of tests/test_gpu_llm_cache.py) on the CPU: it agrees with
oracle/llm_oracle.py's cache (pinned by the reference's goldens in tests/test_llm_oracle.py) over several forward calls
into one cache, and its comparison flags each planted fault by at least 10x the bar while passing the f32 oracle's
own cache."""
import numpy as np
import pytest

from oracle import llm_oracle
from tests import llm_ref64 as R
from tests import synth

QK = 3.0   # q / k weight scale of the attention cases: peaked attention, so a mask or head error is not averaged away


def _oracle_cache(t, cfg, blocks):
    orc = llm_oracle.LlmOracle(t, cfg)
    cache = orc.new_cache()
    for ids in blocks:
        orc.forward(ids, cache)
    return cache


def _blocks(cfg, sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(4, cfg["vocab_size"], n).tolist() for n in sizes]


def _worst(errs):
    """Largest err / bar over layers and K / V."""
    return max(e / b for e, b in errs.values())


def _faulted(ref_cls, t, cfg, blocks):
    ref = ref_cls(t, cfg)
    cache = ref.new_cache()
    for ids in blocks:
        ref.forward(ids, cache)
    return cache


@pytest.mark.parametrize("base,qk", [(synth.LLAMA_TEST, 1.0), (synth.QWEN_TEST, 1.0), (synth.LLAMA_TEST, QK), (synth.QWEN_TEST, QK)],
                         ids=["llama", "qwen2", "llama-peaked", "qwen2-peaked"])
def test_reference_matches_the_oracle_cache(base, qk):
    cfg = dict(base)
    t = synth.llm_tensors(cfg, seed=3, qk_scale=qk)
    blocks = _blocks(cfg, (5, 1, 11, 30, 1, 3))      # several calls appending to one cache
    ref = R.run(t, cfg, blocks)
    assert ref[0][0].shape == (51, cfg["num_key_value_heads"] * 16)
    errs = R.cache_errors(_oracle_cache(t, cfg, blocks), ref)
    assert len(errs) == 2 * cfg["num_hidden_layers"]
    assert _worst(errs) <= 0.1, errs                    # ten times inside the bar the GPU is held to


# ---- planted faults: each is flagged by >= 10x the bar, and the f32 oracle's cache of the same run passes

def _fault_case(fault_ref=None, perturb=None, sizes=(40, 1, 1), qk=QK, base=synth.LLAMA_TEST, **over):
    cfg = dict(base, **over)
    t = synth.llm_tensors(cfg, seed=7, qk_scale=qk)
    blocks = _blocks(cfg, sizes, seed=1)
    ref = R.run(t, cfg, blocks)
    assert _worst(R.cache_errors(_oracle_cache(t, cfg, blocks), ref)) <= 1.0
    bad = _faulted(fault_ref or R.Ref64, t, cfg, blocks)
    if perturb:
        perturb(bad)
    return R.cache_errors(bad, ref)


def test_fault_rows_swapped_at_the_chunk_boundary():
    def swap(cache):
        for K, V in cache:
            K[[2047, 2048]] = K[[2048, 2047]]
            V[[2047, 2048]] = V[[2048, 2047]]
    errs = _fault_case(perturb=swap, sizes=(2050, 1), max_position_embeddings=2560)
    assert _worst(errs) >= 10, errs


def test_fault_rope_one_position_late():
    class Late(R.Ref64):
        def positions(self, offset, rows, layer):
            pos = super().positions(offset, rows, layer)
            return np.where(pos == 23, 24, pos)          # one row rotated at r + 1
    errs = _fault_case(Late)
    assert _worst(errs) >= 10, errs


def test_fault_causal_mask_off_by_one_in_layer_0():
    class Peek(R.Ref64):
        def visible(self, qpos, total, layer):
            if layer:
                return super().visible(qpos, total, layer)
            return np.arange(total)[None, :] <= qpos[:, None] + 1    # each query also sees the next key
    errs = _fault_case(Peek)
    assert errs[(0, "k")][0] == 0 and errs[(0, "v")][0] == 0     # layer 0's K / V are written before its attention
    assert max(errs[(1, "k")][0] / errs[(1, "k")][1], errs[(1, "v")][0] / errs[(1, "v")][1]) >= 10, errs


def test_fault_query_head_reads_the_wrong_kv_head():
    class Wrong(R.Ref64):
        def kv_head_of(self, head):
            g = super().kv_head_of(head)
            return (g + 1) % self.kv_heads if head == 1 else g
    errs = _fault_case(Wrong)
    assert _worst(errs) >= 10, errs


def test_fault_projection_activations_rounded_to_bf16():
    class Bf16(R.Ref64):   # what a three-piece split that drops its lower pieces computes
        def linear(self, x, name, layer):
            if name == "k_proj":
                x = llm_oracle.bf16_round(x.astype(np.float32)).astype(np.float64)
            return super().linear(x, name, layer)
    errs = _fault_case(Bf16, qk=1.0)
    assert _worst(errs) >= 10, errs


def test_fault_row_never_written():
    def zero(cache):
        for K, V in cache:
            K[17] = 0.0
            V[17] = 0.0
    errs = _fault_case(perturb=zero, qk=1.0)
    assert _worst(errs) >= 10, errs


def test_comparison_rejects_a_short_cache_and_non_finite_values():
    cfg = dict(synth.LLAMA_TEST)
    t = synth.llm_tensors(cfg, seed=2)
    ref = R.run(t, cfg, _blocks(cfg, (9,)))
    with pytest.raises(AssertionError):
        R.cache_errors([(k[:-1], v[:-1]) for k, v in ref], ref)
    bad = [(k.copy(), v.copy()) for k, v in ref]
    bad[1][1][4, 0] = np.nan
    assert R.cache_errors(bad, ref)[(1, "v")][0] == float("inf")
    assert R.first_bad_row(bad[1][1], ref[1][1], 1e-4) == 4


def test_rope_frequencies_are_correctly_rounded_powf():
    """theta^(2i/d) as libm's powf rounds it (the reference's f32::powf; the device's host tables, llm.cpp): numpy's
    float32 power was one ulp off at these i, which at position 2 300 turned the angle by ~1e-4 rad."""
    inv = llm_oracle.rope_inv_freq(64, 500000.0)
    assert [inv[1], inv[3], inv[19]] == [np.float32(float.fromhex(h)) for h in ("0x1.53c38cp-1", "0x1.2b3dc6p-2", "0x1.b15902p-12")]
