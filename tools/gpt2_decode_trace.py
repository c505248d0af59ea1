"""gpt2-small shape, bf16 weights: a 128-token prompt, then 64 greedy decode tokens -- the run the committed
rocprofv3 --kernel-trace --stats profile of the GPT-2 decode step comes from:
    rocprofv3 --kernel-trace --stats -d OUT -o gpt2 -- python tools/gpt2_decode_trace.py"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kjarni_amd  # noqa: E402
from tests import gpt2_fixture  # noqa: E402

with tempfile.TemporaryDirectory() as tmp:
    cfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
    gpt2_fixture.gpt2_model(tmp, cfg, seed=0, store_bf16=True, buffers=False, std=0.02)
    dec = kjarni_amd.HipDecoder(tmp)
    out = dec.generate(np.random.default_rng(0).integers(0, 50257, 128).tolist(), 65)  # the first token comes from the prefill
    print(f"generated {len(out)} tokens: 1 from the prefill, {len(out) - 1} graph-replayed decode steps")
