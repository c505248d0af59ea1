"""Llama-3.2-1B shape as an FP8 (e4m3, per-channel scales) checkpoint, the codes kept in HBM: a 128-token prompt, then 64 greedy
decode tokens -- the run the committed rocprofv3 --kernel-trace --stats profile of the FP8 decode step comes from:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fp8 -- python tools/fp8_decode_trace.py"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kjarni_amd  # noqa: E402
from tests import fp8_fixture, synth  # noqa: E402

with tempfile.TemporaryDirectory() as tmp:
    cfg = dict(synth.LLAMA_1B, max_position_embeddings=4096, eos_token_id=synth.LLAMA_1B["vocab_size"] + 1)
    fp8_fixture.fp8_model(tmp, cfg, "channel", seed=0, keep_hf=False)
    dec = kjarni_amd.HipDecoder(tmp, max_context=2048)
    out = dec.generate(np.random.default_rng(0).integers(1000, 100000, 128).tolist(), 65)  # the first token comes from the prefill
    print(f"generated {len(out)} tokens: 1 from the prefill, {len(out) - 1} graph-replayed decode steps")
