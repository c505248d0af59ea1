#!/usr/bin/env python3
"""Seeds for tests/test_gpu_gen_logprobs.py, found with the float64 references alone (no GPU).

A loop case compares top-k ids only in slots whose float64 logit is at least lanes_cases.GAP away from both neighbours of the
sorted list, and may leave out at most 2 % of its slots (none below 50 slots).  This tool walks (model seed, prompt seed) pairs
of a family, runs the reference's greedy trace and prints, per pair, the smallest gap between the two best logits (the ids are
only comparable at all where it clears GAP) and the slots a case of that pair would leave out at each top_k.

    python tools/gen_logprobs_seed_search.py greedy [family ...]     37-token greedy cases (llama, gpt2, qwen3; f32 and bf16)
    python tools/gen_logprobs_seed_search.py wide                    the 72 prompts of tests/wide_cases.py at top_k 4
"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import gen_logprobs_ref64 as R  # noqa: E402
from tests import lanes_cases as LC  # noqa: E402
from tests import wide_cases as WC  # noqa: E402


def left_out(rows, n, k):
    clear = np.array([R.clear_slots(rows[i], k, LC.GAP) for i in range(n)])
    return int(clear.size - clear.sum()), int(clear.size)


def reference(family, seed, bf16, tmp):
    """The test's own fixture builder, without the decoder."""
    from tests import gpt2_fixture as G
    from tests import sampled_lookup_cases as SC
    from tests import synth
    d = os.path.join(tmp, f"{family}-{seed}-{int(bf16)}")
    if family == "gpt2":
        cfg = G.gpt2_config(**G.SMALL)
        _, t = G.gpt2_model(d, cfg, seed=seed, store_bf16=bf16)
        return SC.Gpt264(t, cfg)
    if family == "qwen3":
        from tests import qwen3_fixture as Q3
        from tests.qwen3_ref64 import Qwen3Ref64
        cfg, t = Q3.qwen3_model(d, Q3.Q3_SMALL, seed=seed, store_bf16=bf16)
        return R.Qwen3Logits(Qwen3Ref64(t, cfg), cfg)
    cfg, t = synth.llm_model(d, synth.LLAMA_TEST, seed=seed, store_bf16=bf16)
    return SC.Llama64(t, cfg)


def greedy(families):
    with tempfile.TemporaryDirectory() as tmp:
        for family in families:
            for bf16 in (False, True):
                for mseed in range(1, 8):
                    ref = reference(family, mseed, bf16, tmp)
                    for pseed in range(1, 6):
                        prompt = np.random.default_rng(pseed).integers(ref.first_id, ref.vocab, 9).tolist()
                        tr = R.greedy_trace(ref, prompt, 37, stops=[ref.vocab - 1])
                        n = len(tr["ids"])
                        gap = min(float(np.diff(np.sort(r)[-2:])[0]) for r in tr["rows"][:n]) if n else 0.0
                        out8 = left_out(tr["rows"], n, 8)
                        ok = n == 37 and gap >= LC.GAP and out8[0] <= int(0.02 * out8[1])
                        print(f"{family} bf16 {int(bf16)} model {mseed} prompt {pseed}: tokens {n} gap {gap:.2e} left out {out8[0]} / {out8[1]}"
                              f"{'  <- ok' if ok else ''}", flush=True)
                        if ok:
                            break
                    else:
                        continue
                    break


def wide():
    from tests import sampled_lookup_cases as SC
    seed, cfg, t, ps, news = WC.case_set("llama")
    ref = SC.Llama64(t, cfg)
    slots = out = 0
    for p, m in zip(ps, news):
        tr = R.greedy_trace(ref, p, int(m), stops=cfg["eos_token_id"] if isinstance(cfg["eos_token_id"], list) else [cfg["eos_token_id"]])
        o, s = left_out(tr["rows"], len(tr["ids"]), 4)
        slots, out = slots + s, out + o
    print(f"wide llama seed {seed}: left out {out} / {slots} ({100.0 * out / max(slots, 1):.2f} %)")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "greedy"
    if what == "wide":
        wide()
    else:
        greedy(sys.argv[2:] or ["llama", "gpt2", "qwen3"])
