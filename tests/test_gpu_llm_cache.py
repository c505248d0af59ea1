"""Every KV-cache row of every layer of the decoder-only path (kjarni_hip_decoder_*) against the float64 reference of
tests/llm_ref64.py, after each forward / generate call.  For layers 0 .. L-2 the next layer's K / V row of a position is
a function of that layer's whole output row, so comparing all rows checks every route for every position, not only the
last rows that test_gpu_llm.py sees.  The bar is test_gpu_llm.py's: max |gpu - ref| <= 1e-4 * max(1, max |ref|), per
layer and per K / V.  Each case names the route it exercises and the condition in kjarni_amd/csrc that selects it."""
import numpy as np
import pytest

from tests import llm_ref64 as R
from tests import synth
from tests.parity_report import report

pytestmark = pytest.mark.gpu
QK = 2.0   # q / k weight scale of the attention cases (synth.llm_tensors): peaked attention, so a masking error shows


class _Pair:
    """One synthetic model on the GPU and in the float64 reference, fed the same token blocks."""

    def __init__(self, tmp_path, case, base, seed=0, weights="auto", max_context=0, **kw):
        import kjarni_amd
        d = str(tmp_path / "model")
        self.case = case
        self.cfg, t = synth.llm_model(d, base, seed=seed, **kw)
        self.ref = R.Ref64(t, self.cfg)
        self.cache = self.ref.new_cache()
        self.gpu = kjarni_amd.HipDecoder(d, weights=weights, max_context=max_context)
        self.rng = np.random.default_rng(seed + 100)

    def ids(self, n):
        return self.rng.integers(4, self.cfg["vocab_size"], n).tolist()

    def forward(self, n):
        ids = self.ids(n)
        self.ref.forward(ids, self.cache)
        self.gpu.forward(ids, fetch=False)
        self.check(f"{len(self.cache[0][0])}")

    def check(self, tag):
        """Every row [0, cache_len) of every layer's K and V against the reference."""
        n = self.cache[0][0].shape[0]
        assert self.gpu.cache_len() == n, (tag, self.gpu.cache_len(), n)
        got = [self.gpu.kv_rows(i) for i in range(len(self.cache))]
        errs = R.cache_errors(got, self.cache)
        bad = []
        for (i, kv), (err, bar) in sorted(errs.items()):
            report(f"llm_cache/{self.case}/layer{i}.{kv}", err, bar)
            if not err <= bar:
                j = "kv".index(kv)
                bad.append((i, kv, err, bar, R.first_bad_row(got[i][j], self.cache[i][j], bar)))
        assert not bad, f"{self.case} after {tag} rows: (layer, k|v, max err, bar, first bad row) {bad}"


@pytest.mark.parametrize("base", [synth.LLAMA_TEST, synth.QWEN_TEST], ids=["llama-d16-gqa2", "qwen2-bias-mqa"])
def test_short_blocks_on_8_row_passes(tmp_path, base):
    """Blocks of fewer than 24 rows (LlmModel::forward, n < kMinGemmRows) run pass() 8 rows at a time: the 8-row
    norm + QKV GEMV writing K / V straight into the cache at row_off = cache_len, launch_rope on the new K rows, the
    decode attention; single tokens take the fused norm + QKV + RoPE launch (pass(), n == 1)."""
    p = _Pair(tmp_path, "8row-" + base["model_type"], base, seed=3, qk_scale=QK)
    for n in (5, 1, 11, 3, 1):
        p.forward(n)


def test_long_prompt_on_8_row_passes(tmp_path):
    """A 40-row prompt with hidden 72 (hidden % 32 != 0: LlmModel::forward does not take prefill_rows) runs as five
    8-row passes, each appending to the cache the next one attends over; 9 heads of 8 over 3 KV heads."""
    base = dict(synth.LLAMA_TEST, hidden_size=72, num_attention_heads=9, num_key_value_heads=3, head_dim=8, intermediate_size=144)
    p = _Pair(tmp_path, "8row-long-h72", base, seed=4, qk_scale=QK)
    for n in (40, 1):
        p.forward(n)


def test_prompt_gemm_with_split_k_and_generic_attention(tmp_path):
    """Blocks of >= 24 rows below 512 go through prefill_rows on the 64 x 64 prompt GEMM (launch_prefill_gemm: K split in
    2 slices, prefill_gemm_ksplit, at K = 256 and 512) and, with fewer than 256 rows, the generic prefill attention
    (prefill_attention_kernel, base = cache_len); single tokens in between; d 64, GQA groups of 2."""
    base = dict(synth.LLAMA_TEST, hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512, head_dim=64)
    p = _Pair(tmp_path, "prefill-gemm-d64-gqa2", base, seed=5, qk_scale=QK)
    for n in (70, 1, 1, 40):
        p.forward(n)


def test_prompt_attention_fallback_for_narrow_heads(tmp_path):
    """Head dim 8: prefill_attention_supported() is false, so prefill_rows runs the decode attention 8 query rows at a
    time over everything cached up to them (the GEMMs stay on the prompt route)."""
    base = dict(synth.LLAMA_TEST, hidden_size=64, num_attention_heads=8, num_key_value_heads=4, head_dim=8, intermediate_size=128)
    p = _Pair(tmp_path, "prefill-d8-fallback", base, seed=6, qk_scale=QK)
    for n in (30, 1, 26):
        p.forward(n)


@pytest.mark.parametrize("head_dim,heads,kv_heads", [(64, 8, 2), (128, 4, 4)], ids=["d64-gqa4", "d128-mha"])
def test_mfma_causal_attention(tmp_path, head_dim, heads, kv_heads):
    """Blocks of >= 256 rows with 64- / 128-wide heads take prefill_attention_mfma_kernel (launch_prefill_attention):
    a first block (base 0), then a 457-row block on top of a 301-row cache (base > 0, ending inside a 128-key chunk),
    with single tokens between."""
    base = dict(synth.LLAMA_TEST, hidden_size=heads * head_dim, num_attention_heads=heads, num_key_value_heads=kv_heads,
                intermediate_size=512, vocab_size=600, max_position_embeddings=2048, head_dim=head_dim)
    base["rope_scaling"] = dict(base["rope_scaling"], original_max_position_embeddings=512)
    p = _Pair(tmp_path, f"mfma-attention-d{head_dim}-h{heads}-kv{kv_heads}", base, seed=7, qk_scale=QK)
    for n in (300, 1, 457, 1):
        p.forward(n)


def test_bf16_weights_on_the_64x64_prompt_gemm(tmp_path):
    """bf16 weights with hidden 160 / inner 288: not 128-multiples, so no projection may take the 128 x 128 tiles
    (prefill_rows' tile_shapes) and the prompt GEMM reads the bf16 weights itself (launch_prefill_gemm, bf16 = 1)."""
    base = dict(synth.LLAMA_TEST, hidden_size=160, num_attention_heads=5, num_key_value_heads=1, head_dim=32, intermediate_size=288)
    p = _Pair(tmp_path, "bf16-prefill-h160", base, seed=8, store_bf16=True, qk_scale=QK)
    assert p.gpu.bf16
    for n in (100, 1, 30):
        p.forward(n)
    assert p.gpu.tile_gemm_calls() == 0


@pytest.mark.parametrize("store_bf16", [False, True], ids=["f32", "bf16"])
def test_tile_gemm_over_two_chunks(tmp_path, store_bf16):
    """Hidden 1 792 = 14 x 128 with a 1 792-wide FFN (the geometry of test_long_prompt_blocks_take_the_tile_gemm): a
    2 300-row prompt is a 2 048-row chunk (kChunk) whose q, o, gate, up and down projections have 16 x 14 = 224 >= 208
    tiles of 128 x 128 (f32: the encoder's f32 GEMM; bf16: the three-piece split on the bf16 matrix cores, K % 64 == 0)
    and a 252-row chunk below the 512-row floor on the 64 x 64 route, on top of the first chunk's cache rows."""
    base = dict(synth.LLAMA_TEST, hidden_size=1792, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2,
                intermediate_size=1792, vocab_size=777, max_position_embeddings=4096, head_dim=128)
    base["rope_scaling"] = dict(base["rope_scaling"], original_max_position_embeddings=1024)
    p = _Pair(tmp_path, "tile-gemm-2chunks-" + ("bf16" if store_bf16 else "f32"), base, seed=13, bf16_values=True,
              store_bf16=store_bf16, std=0.02)
    assert p.gpu.bf16 == store_bf16
    for n in (2300, 1):
        p.forward(n)
    assert p.gpu.tile_gemm_calls() == 5 * base["num_hidden_layers"]


def test_chunk_edge(tmp_path):
    """A 2 049-row prompt: prefill_rows' second chunk holds a single row (cache_len 2 048 as its base), then one token."""
    base = dict(synth.LLAMA_TEST, max_position_embeddings=2304)
    p = _Pair(tmp_path, "chunk-edge-2049", base, seed=9, qk_scale=QK)
    for n in (2049, 1):
        p.forward(n)


@pytest.mark.parametrize("store_bf16", [False, True], ids=["f32", "bf16"])
def test_fused_decode_step_with_the_embedding_folded_in(tmp_path, store_bf16):
    """Hidden 2 048: single tokens run launch_llm_qkv_rope's streaming kernel (llm_qkv_rope_embeds: k in {2048, 4096,
    8192}), whose layer-0 launch also gathers the embedding row (pass(), embed_in_qkv); the prompt before them takes
    prefill_rows."""
    base = dict(synth.LLAMA_TEST, hidden_size=2048, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=8, head_dim=64,
                intermediate_size=256, vocab_size=500, max_position_embeddings=512)
    base["rope_scaling"] = dict(base["rope_scaling"], original_max_position_embeddings=128)
    p = _Pair(tmp_path, "fused-decode-h2048-" + ("bf16" if store_bf16 else "f32"), base, seed=10, bf16_values=True,
              store_bf16=store_bf16, std=0.02)
    p.forward(30)
    for _ in range(5):
        p.forward(1)


def test_graph_replayed_greedy_steps(tmp_path):
    """LlmModel::generate, plain greedy: each step is the captured graph (step_graph) reading the token and the cache
    position from the device (pos_), replayed in bursts.  The cache after generating G tokens holds the prompt and the
    first G - 1 of them; then forward() must append at cache_len again."""
    base = dict(synth.LLAMA_TEST, eos_token_id=[])          # no stop token: all 20 tokens come
    p = _Pair(tmp_path, "greedy-graph", base, seed=11, qk_scale=QK)
    prompt = p.ids(30)
    out = p.gpu.generate(prompt, 20)
    assert len(out) == 20
    p.ref.forward(prompt + out[:-1], p.cache)
    p.check("generate")
    p.forward(3)
    p.forward(1)


def test_context_edge(tmp_path):
    """max_context 64 below the config's 256 (cache_cap_): the cache fills to exactly 64 rows; the next forward raises
    and leaves the cache as it was; reads past cache_len or of a missing layer raise."""
    p = _Pair(tmp_path, "context-edge", synth.LLAMA_TEST, seed=12, max_context=64, qk_scale=QK)
    assert p.gpu.context == 64
    for n in (40, 16, 7, 1):
        p.forward(n)
    assert p.gpu.cache_len() == 64
    with pytest.raises(Exception):
        p.gpu.forward(p.ids(1), fetch=False)
    p.check("a refused forward")
    for bad in (dict(layer=2), dict(layer=-1), dict(layer=0, first=60, rows=5), dict(layer=0, first=65, rows=0)):
        with pytest.raises(Exception):
            p.gpu.kv_rows(**bad)
    k, v = p.gpu.kv_rows(1, 60, 4)
    assert np.array_equal(k, p.gpu.kv_rows(1)[0][60:]) and np.array_equal(v, p.gpu.kv_rows(1)[1][60:])
    p.gpu.reset()
    assert p.gpu.cache_len() == 0
    with pytest.raises(Exception):
        p.gpu.kv_rows(0, 0, 1)
