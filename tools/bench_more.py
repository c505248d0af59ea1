#!/usr/bin/env python3
"""The other measurements SURVEY.md section 8(d) asks for, next to bench.py's headline line.

    python tools/bench_more.py [rerank] [scan] [ragged] [host] [strings] [indexer] [whisper] [llm]   (default: all)

One JSON line per measurement (1 GPU; the N > 1 driver is bench.py):
  rerank   BASELINE.json configs[2] on one GPU: 100 000 synthetic (query, doc) pairs, S = 128, fp32,
           ids/mask/types resident in HBM -> 100 000 logits.  pairs/s + fraction of the fp32 MFMA peak.
  scan     cosine scan + top-10 over unit-norm Gaussian corpora [N, 384], N in {1e5, 1e6, 1e7}, 1 and 64
           queries, corpus resident in HBM.  docs/s and the scan kernel's algorithmic GB/s vs 8 TB/s.
  ragged   the headline embed workload with lengths ~ U{16..128} (right-padded): masking cost.
  host     the headline embed workload through the host-pointer entry point: H2D of ids/mask and D2H of
           the embeddings inside the timed region (the PCIe-inclusive rate; never the headline value).
  strings  kjarni_embedder_encode_batch on generated ASCII sentences (tokenisation on the host included).
  indexer  kjarni_indexer_create over a generated directory tree: chunks/s end to end.
  whisper  BASELINE.json configs[3]: Whisper-base shaped model (random init), 30 s of synthetic audio: log-mel,
           conv stem + encoder, greedy decode of 448 tokens; per-stage ms, x real time, and the CPU restatement
           (oracle) timed on a bounded sample of the same work.
  llm      BASELINE.json configs[4]: Llama-3.2-1B-shaped decoder (random init), weights bf16 in HBM, f32 KV cache:
           prefill of a 128-token prompt and greedy decode of 256 tokens; tokens/s and the weight stream vs HBM peak.
  llm_lanes  (only on request) batched greedy decode, 1 / 2 / 4 / 8 prompts in lock step (HipDecoder.generate_batch) against
           the single-stream generate() of the same build, alternated twice in one process: Llama-3.2-1B shape (bf16),
           gpt2-small (bf16, f32) and the 1B shape as a GGUF Q4_K_M-style mix; 128-token prompts; aggregate tokens/s and
           ms per lock-step step.  KJARNI_LANES_STEPS=N: N steps at 8 lanes on the Llama shape only (for a kernel trace).
  llm_wide   (only on request) wide lanes: generate_wide at 16 / 32 / 64 prompts in lock step against single-stream generate()
           and generate_batch at 8 lanes of the same build (the baselines), twice in one process: Llama-3.2-1B shape (bf16) and
           gpt2-small (bf16); 128-token prompts, 128 new tokens, lane_context 512; aggregate tokens/s and ms per step.
           KJARNI_WIDE_STEPS=N: N steps at 64 lanes on the Llama shape only (for a kernel trace).
  llm_lookup  (only on request) prompt-lookup decoding against plain generate() of the same build, alternated twice in one
           process: Llama-3.2-1B shape (bf16) and gpt2-small (bf16); ms per plain step, ms per verify step at 2 / 4 / 8 rows
           (HipDecoder.verify_step in a loop with a fixed draft, and the replayed graph inside generate_lookup), the break-even
           acceptance verify_ms / plain_ms - 1, and end-to-end tokens/s with the acceptance histogram -- on a random-init
           model, whose greedy output degenerates into repetition: the full-acceptance end of the range, not a workload.
           KJARNI_LOOKUP_STEPS=N: N verify steps of 8 rows on the Llama shape only (for a kernel trace).
  llm_lookup_sampled  (only on request) prompt-lookup decoding for sampled requests against the plain sampled loop of the same
           build, alternated twice in one process, at the family's default sampling config: Llama-3.2-1B shape (bf16) and
           gpt2-small (bf16); ms per plain sampled step, ms per verify-and-cut step at 2 / 4 / 8 rows (HipDecoder.
           verify_step_sampled in a loop), the break-even acceptance, and tokens/s at both ends of acceptance (draws of 0 take
           token 0: everything drafted is accepted; seeded draws on a random-init model: next to nothing is).
  llm_draft  (only on request) speculative decoding with a draft model (HipDecoder.generate_draft) on the Llama-3.2-1B shape (bf16)
           as target, against plain generate() of the same build, alternated twice in one process: ms per round at 2 / 4 / 8
           rows from the replayed chain, next to the target's plain step and to the verify step of the same row count plus
           (rows - 1) drafter steps (what the chain is made of), the break-even accepted tokens per round, and end-to-end
           tokens/s with a copy of the target as drafter (every draft accepted) and with an unrelated checkpoint; a 4-layer
           drafter of the same width for the per-round cost only.  Ends of a range, not workloads.
  llm_moe  (only on request) a random-weight qwen3_moe model at the Qwen3-30B-A3B widths (128 experts of 768, 8 per token, bf16, cut
           to 4 layers: a 5 GB fixture) against a dense Qwen3 model of the same widths with intermediate_size 6144 (the same active
           FFN bytes and FLOPs) in one process, alternated twice: greedy ms / token and the 128-token prompt time of both, their
           ratios, and the sparse step's streamed bytes against the HBM peak.
  llm_logprobs  (only on request) generation log-probabilities (HipDecoder.generate_logprobs / generate_wide_logprobs) against the same
           loop with them off: greedy and sampled, top_k 0 and 8, on the Llama-1B and gpt2-small shapes; 64 wide lanes off and on;
           the kernel pair alone at V = 128 256 / 151 936 for 1 and 64 rows against the one-workgroup-per-row score kernel on the same
           rows.  The lines also go to profiles/llm_logprobs_bench.jsonl.
  llm_constraint  (only on request) constrained decoding (HipDecoder.generate_constrained) against the plain loop of the same build,
           alternated twice in one process, greedy and sampled: Llama-3.2-1B shape (bf16) and gpt2-small (bf16), a pattern that
           masks nothing (the ids are the plain loop's, asserted), so the ratio is the cost of the two launches per step; and the
           mask build of a 100-state pattern at each shape's vocabulary.  The lines also go to profiles/llm_constraint_bench.jsonl.
  llm_grammar  (only on request) grammar-constrained decoding (HipDecoder.generate_grammar) against the pattern route and the plain
           loop of the same run, Llama-3.2-1B and gpt2-small shapes, greedy and sampled; json_value on random weights and the device
           object's constructor at V = 128 256 for information.  The lines also go to profiles/llm_grammar_bench.jsonl.
  llm_wide_constraint  (only on request) constrained decoding in 64 wide lanes (HipDecoder.generate_wide_constrained) against plain
           generate_wide of the same run, alternated twice: a pattern that masks nothing and the one-rule grammar of the same
           language in every lane, Llama-3.2-1B and gpt2-small shapes (bf16), 128-token prompts, 128 new tokens, lane_context 512;
           tokens/s and ms per step of each leg, the spread, the added launches' time per step; json_value at 64 lanes on random
           weights for information.  The lines also go to profiles/llm_wide_constraint_bench.jsonl.
  llm_wide_fp8  (only on request) FP8 checkpoints on the matrix cores (HipDecoder.set_fp8_matrix_cores): generate_wide at 16 / 32 / 64
           lanes with the switch on against FP8 generate_batch at 8 lanes and against a bf16 load of the same shape at the same
           widths, and the prompt's time at 128 / 384 tokens with the switch off, on and for bf16; Llama-3.2-1B shape (per-channel
           scales) and Qwen3-0.6B shape (block scales), every leg twice, best of two.  The lines also go to
           profiles/llm_wide_fp8_bench.jsonl.
  llm_score  (only on request) HipDecoder.score() against forward() of the same ids in one process, alternated twice: Llama-3.2-1B
           shape (bf16) and gpt2-small (bf16), prompts of 128 and 2 048 tokens, first = 1, on the fused route (the head on the
           matrix cores, no logits stored) and on the rows route (8 materialised logits rows at a time); medians of runs that
           end in a synchronise; the head's added time score - forward per route.
           KJARNI_SCORE_TRACE=N: N fused score() calls of the 2 048-token prompt on the Llama shape only (for a kernel trace).
  llm_score_topk  (only on request) HipDecoder.score_topk() at top_k = 1 and 8 against score() of the same ids in one process,
           alternated twice: Llama-3.2-1B shape (bf16), prompts of 128 and 2 048 tokens, first = 1, on the fused and on the rows
           route; medians of runs that end in a synchronise; the ratio score_topk / score per case.  One line per (length,
           route); the lines also go to profiles/llm_score_topk_bench.jsonl.
  llm_score_batch  (only on request) HipDecoder.score_batch() -- many sequences scored in one packed pass, shared contexts computed
           once -- on the Llama-3.2-1B shape (bf16, random init), legs alternated twice in one process, medians of runs that end in a
           synchronise: N x 128 tokens at first = 1 for N in 8 / 64 / 256 against a loop of score() over the same sequences; 64
           contexts x 4 continuations of 16 tokens with contexts of 256 / 64 / 16 / 4 / 1 tokens, as given (sharing) against the
           same batch with every sequence's token 0 made distinct (same shapes, nothing shared), and at 256 the score() loop;
           the 64- and 16-token cases behind a first token common to all sequences against a first token per context.
           The lines also go to profiles/llm_score_batch_bench.jsonl.
  llm_prefix  (only on request) prefix reuse off against on (HipDecoder.set_prefix_reuse) in one process, alternated twice:
           Llama-3.2-1B shape (bf16) and gpt2-small (bf16).  Time to the first token of turn 2 with a resident history of 512 /
           2 048 tokens and a 32-token message; five score() calls over one 512-token context with 8-token continuations; 8
           requests under a 512-token shared prefix on 8 lanes (16-token tails, 16 new tokens), with the prefix not resident
           and resident.  Medians of runs that end in a synchronise; the lines also go to profiles/llm_prefix_bench.jsonl.
  llm_qwen3  (only on request) the Qwen3-0.6B shape (hidden 1024, 28 layers, 16 / 8 heads of 128, intermediate 3072, vocab
           151 936, tied head, bf16 weights, random init): 128-token prompt time, greedy decode of 256 tokens; tokens/s and
           ms per token (six launches per layer: the per-head Q / K norm + RoPE is a launch of its own).  The line also goes
           to profiles/qwen3_bench_llm.jsonl.  KJARNI_QWEN3_TRACE=N: a 128-token prompt and N decode steps only (for a
           kernel trace).
  llm_embed  (only on request) HipDecoder.embed() -- decoder embedders, last-token pooling over packed batches -- on the Qwen3-0.6B
           shape (bf16, random init): sentences/s for 4 096 x 128 tokens and for 4 096 ragged sentences of U{16..128} tokens,
           the latency of 1, 8 and 64 x 128, and in the same run a loop of forward() + last_hidden() per sentence (what there
           was before embed()) over the same 64 x 128, alternated twice; medians of runs that end in a synchronise.  The lines
           also go to profiles/decoder_embed_bench.jsonl.
  llm_rerank  (only on request) HipDecoder.answer_logits() -- decoder rerankers: two chosen logits at the end of many prompts in one
           packed pass, the query computed once -- on the Qwen3-0.6B shape (bf16, random init): one query of 64 tokens in front of
           16 / 64 / 256 documents of 128 tokens, as given (sharing) against the same batch with every sequence's token 0 made
           distinct (nothing shared) and against a loop of forward() over the same sequences; legs alternated twice, medians of
           runs that end in a synchronise.  The lines also go to profiles/decoder_rerank_bench.jsonl.
"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
S = 128


def flops_per_row(H=384, L=6, I=1536, seq=S, head=0):
    per_layer = 2 * seq * H * 3 * H + 2 * 2 * seq * seq * H + 2 * seq * H * H + 2 * 2 * seq * H * I
    return L * per_layer + head


def usable_cores():
    """Threads for a CPU leg: physical cores, capped by the affinity mask and the cgroup CPU quota (as bench.py's)."""
    try:
        import psutil
        n = psutil.cpu_count(logical=False) or os.cpu_count() or 1
    except Exception:
        n = os.cpu_count() or 1
    if hasattr(os, "sched_getaffinity"):
        n = min(n, len(os.sched_getaffinity(0)))
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def timed(fn, sync, steps, warmup):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t0) / steps


def main():
    which = set(sys.argv[1:]) or {"rerank", "scan", "ragged", "host", "sweep", "strings", "latency", "families", "indexer", "search", "whisper", "llm", "chat", "gpt2"}  # "llm8b" only on request (writes 16 GB)
    import numpy as np
    import torch

    import kjarni_amd
    from kjarni_amd import _ffi
    from tests import synth

    assert torch.cuda.is_available() and kjarni_amd.device_count() >= 1, "needs an AMD GPU"
    dev = torch.device("cuda", 0)
    L = _ffi.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    sync = torch.cuda.synchronize

    def emit(d):
        print(json.dumps(d), flush=True)

    tmp = tempfile.mkdtemp(prefix="kjarni_bench_more_")
    emb_dir = os.path.join(tmp, "cache", "sentence-transformers_all-MiniLM-L6-v2")
    cfg, _ = synth.minilm_embedder(emb_dir, seed=0)
    synth.add_tokenizer(emb_dir)

    if "rerank" in which:
        d = os.path.join(tmp, "ce")
        cfg_r, _ = synth.minilm_cross_encoder(d, seed=1)
        enc = kjarni_amd.HipEncoder(d, 0)
        N = 100_000
        ids, mask, types = synth.synthetic_pairs(N, S, seed=1)
        t_ids, t_mask, t_types = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (ids, mask, types))
        out = torch.empty((N, enc.num_labels), dtype=torch.float32, device=dev)
        dt = timed(lambda: enc.logits_dev(t_ids.data_ptr(), t_mask.data_ptr(), t_types.data_ptr(), N, S, out.data_ptr(),
                                          stream=stream()), sync, steps=3, warmup=1)
        fl = flops_per_row(head=2 * 384 * 384 + 2 * 384)
        emit({"metric": "pairs/sec minilm-l6-v2-cross-encoder rerank (seq=128)", "value": round(N / dt, 1), "unit": "pairs/s",
              "n_gpus": 1, "ms_per_step": round(dt * 1e3, 2), "dtype": "f32", "data": "synthetic",
              "config": {"workload": "BASELINE.json configs[2] on one GPU: 100 000 synthetic query-doc pairs, seq_len=128"},
              "e2e_tflops": round(N / dt * fl / 1e12, 2),
              "e2e_frac_fp32_mfma_peak": round(N / dt * fl / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)})
        del enc, t_ids, t_mask, t_types, out

    if "families" in which:
        # The other registry embedders at their real shapes (random weights): nomic-embed-text-v1.5 (RoPE + SwiGLU, 768 x 12
        # layers, inner 3072), all-mpnet-base-v2 (BERT-base shape) and bge-m3 (XLM-R large: 1024 x 24 layers, inner 4096,
        # 250 002-row embedding table, up to 8 192 tokens).  Same token-level entry point as the headline.
        for name, make, over, gated in (
                ("nomic-embed-text", synth.nomic_embedder, dict(n_embd=768, n_layer=12, n_head=12, n_inner=3072, n_positions=8192), True),
                ("mpnet-base-v2", synth.mpnet_embedder, dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                                             intermediate_size=3072), False),
                ("bge-m3", synth.xlmr_embedder, dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                                                     vocab_size=250002, max_position_embeddings=8194), False)):
            d = os.path.join(tmp, name)
            cfg_f, _ = make(d, **over)
            enc = kjarni_amd.HipEncoder(d, 0)
            H = cfg_f.get("hidden_size", cfg_f.get("n_embd"))
            Lf = cfg_f.get("num_hidden_layers", cfg_f.get("n_layer"))
            If = cfg_f.get("intermediate_size", cfg_f.get("n_inner"))
            shapes = ((16384, 128), (1024, 2048)) if gated else ((8192, 128), (256, 8192)) if name == "bge-m3" else ((16384, 128), (4096, 512))
            for N, seq in shapes:
                ids, mask = synth.synthetic_ids(N, seq, vocab=cfg_f["vocab_size"], seed=0)
                t_ids, t_mask = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (ids, mask))
                out = torch.empty((N, H), dtype=torch.float32, device=dev)
                run = lambda: enc.embed_dev(t_ids.data_ptr(), t_mask.data_ptr(), N, seq, out.data_ptr(), stream=stream())  # noqa: E731
                dt = timed(run, sync, steps=2, warmup=1)
                enc.profile_begin()
                run()
                stats = [k for k in enc.profile_end() if k["launches"]]
                ffn = (3 if gated else 2) * 2 * seq * H * If
                fl = Lf * (2 * seq * H * 3 * H + 4 * seq * seq * H + 2 * seq * H * H + ffn)
                emit({"metric": f"sentences/sec {name} batch encode (seq={seq})", "value": round(N / dt, 1), "unit": "sentences/s",
                      "n_gpus": 1, "ms_per_step": round(dt * 1e3, 2), "dtype": "f32", "data": "synthetic",
                      "config": {"workload": f"{N} sentences x {seq} tokens, ids/mask in HBM, mean pool + L2"},
                      "tokens_per_s": round(N * seq / dt, 0), "e2e_tflops": round(N / dt * fl / 1e12, 2),
                      "e2e_frac_fp32_mfma_peak": round(N / dt * fl / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4),
                      "kernels": [{"kind": k["kind"], "launches": k["launches"], "ms": round(k["total_ms"], 2),
                                   "tflops": round(k["flops"] / k["total_ms"] / 1e9, 1) if k["flops"] else None,
                                   "gbs": round(k["bytes"] / k["total_ms"] / 1e6, 0)} for k in stats]})
                del t_ids, t_mask, out
            del enc

    if "ragged" in which or "host" in which:
        enc = kjarni_amd.HipEncoder(emb_dir, 0)
        N = 65536
        if "ragged" in which:
            ids, mask = synth.synthetic_ids(N, S, seed=0, ragged=True)
            t_ids, t_mask = (torch.from_numpy(a.view(np.int32)).to(dev) for a in (ids, mask))
            out = torch.empty((N, 384), dtype=torch.float32, device=dev)
            # device-pointer calls keep the padded layout unless the caller opts in (mode 2 reads the lengths back and
            # synchronises the stream once per call: include/kjarni_hip.h); both are reported
            dt_padded = timed(lambda: enc.embed_dev(t_ids.data_ptr(), t_mask.data_ptr(), N, S, out.data_ptr(), stream=stream()),
                              sync, steps=2, warmup=1)
            enc.set_packing(2)
            dt = timed(lambda: enc.embed_dev(t_ids.data_ptr(), t_mask.data_ptr(), N, S, out.data_ptr(), stream=stream()),
                       sync, steps=3, warmup=1)
            enc.set_packing(1)
            emit({"metric": "sentences/sec minilm-l6-v2 batch encode (seq=128), ragged lengths U{16..128} right-padded",
                  "value_padded_layout": round(N / dt_padded, 1),
                  "value": round(N / dt, 1), "unit": "sentences/s", "n_gpus": 1, "ms_per_step": round(dt * 1e3, 2),
                  "dtype": "f32", "data": "synthetic", "config": {"workload": "65 536 sentences padded to 128, mean length 72"},
                  "real_tokens_per_s": round(float(mask.sum()) / dt, 0)})
            del t_ids, t_mask, out
        if "host" in which:
            ids, mask = synth.synthetic_ids(N, S, seed=0)
            dt = timed(lambda: enc.embed(ids, mask), lambda: None, steps=2, warmup=1)
            emit({"metric": "sentences/sec minilm-l6-v2 batch encode (seq=128), host pointers (H2D ids/mask + D2H embeddings timed)",
                  "value": round(N / dt, 1), "unit": "sentences/s", "n_gpus": 1, "ms_per_step": round(dt * 1e3, 2),
                  "dtype": "f32", "data": "synthetic",
                  "config": {"workload": "65 536 sentences x 128 through kjarni_hip_encoder_embed_host (pageable host memory)"}})
        del enc

    if "sweep" in which:
        # Calls of the sizes real callers make (the reference's default batch is 32, kjarni-ffi/src/embedder.rs): host
        # pointers in and out, one call at a time, sentences/s against the call size and the padded length.
        enc = kjarni_amd.HipEncoder(emb_dir, 0)
        rows = []
        for seq in (32, 128):
            for b in (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096):
                ids, mask = synth.synthetic_ids(b, seq, seed=1)
                reps = max(3, min(200, 4096 // b))
                for _ in range(50 if not rows else 1):  # (the first size also absorbs the clock ramp from idle)
                    enc.embed(ids, mask)
                t0 = time.perf_counter()
                for _ in range(reps):
                    enc.embed(ids, mask)
                dt = (time.perf_counter() - t0) / reps
                rows.append({"batch": b, "seq": seq, "ms_per_call": round(dt * 1e3, 4), "sentences_per_s": round(b / dt, 1),
                             "frac_fp32_mfma_peak": round(b * flops_per_row(seq=seq) / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4)})
        emit({"metric": "sentences/sec minilm-l6-v2 embed against the call size (host pointers, one call at a time)",
              "unit": "sentences/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic", "value": rows[-1]["sentences_per_s"],
              "config": {"workload": "kjarni_hip_encoder_embed_host, batch 1 .. 4096 x seq 32 / 128"}, "calls": rows})
        del enc

    if "scan" in which:
        dim, k = 384, 10
        for n in (100_000, 1_000_000, 10_000_000):
            g = torch.Generator(device=dev).manual_seed(2)
            corpus = torch.randn((n, dim), generator=g, device=dev, dtype=torch.float32)
            corpus /= torch.linalg.vector_norm(corpus, dim=1, keepdim=True)
            for nq in (1, 64):
                q = torch.randn((nq, dim), generator=g, device=dev, dtype=torch.float32)
                scores = torch.empty((nq, n), dtype=torch.float32, device=dev)
                ws = torch.empty(L.kjarni_hip_cosine_topk_workspace_bytes(nq, n, k), dtype=torch.uint8, device=dev)
                idx = torch.empty((nq, k), dtype=torch.int64, device=dev)
                sc = torch.empty((nq, k), dtype=torch.float32, device=dev)

                def scan():
                    _ffi.check_error(L.kjarni_hip_cosine_scores(0, q.data_ptr(), nq, corpus.data_ptr(), n, dim, 1,
                                                                scores.data_ptr(), stream()))

                def topk():
                    _ffi.check_error(L.kjarni_hip_cosine_topk(0, scores.data_ptr(), nq, n, k, ws.data_ptr(), idx.data_ptr(),
                                                              sc.data_ptr(), stream()))
                steps = 20 if n <= 1_000_000 else 5
                t_scan = timed(scan, sync, steps, 2)
                t_topk = timed(topk, sync, steps, 2)
                t_all = timed(lambda: (scan(), topk()), sync, steps, 2)
                two_idx, two_sc = idx.clone(), sc.clone()
                # the one-call form (kjarni_hip_cosine_search): for one query a single fused pass, no score array
                ws2 = torch.empty(L.kjarni_hip_cosine_search_workspace_bytes(nq, n, dim, k), dtype=torch.uint8, device=dev)

                def search():
                    _ffi.check_error(L.kjarni_hip_cosine_search(0, q.data_ptr(), nq, corpus.data_ptr(), n, dim, 1, k, ws2.data_ptr(),
                                                                idx.data_ptr(), sc.data_ptr(), stream()))
                t_search = timed(search, sync, steps, 2)
                fused_equal = bool(torch.equal(idx, two_idx)) and bool(torch.equal(sc, two_sc))
                del ws2
                ref_idx = torch.topk(q @ corpus.T if n <= 1_000_000 else scores, k, dim=1).indices
                same = bool(torch.equal(torch.sort(ref_idx, dim=1).values, torch.sort(idx, dim=1).values))
                alg = n * dim * 4
                if nq < 20:   # one streaming pass over the corpus per group of 4 queries: HBM-bound
                    passes = (nq + 3) // 4
                    roof = {"kernel": "cosine_scores_stream_kernel", "bound": "hbm",
                            "achieved": round(alg * passes / t_scan / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": round(alg * passes / t_scan / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                            "algorithmic_bytes_per_launch": alg, "launches_per_scan": passes}
                else:         # the fused matrix-core scan: dots, document norms and cosines in one launch per 64 queries
                    fl = 2.0 * nq * n * dim
                    roof = {"kernel": "cosine_scan_mfma_kernel", "bound": "mfma",
                            "achieved": round(fl / t_scan / 1e12, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                            "frac": round(fl / t_scan / 1e12 / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": None,
                            "algorithmic_flops": fl, "corpus_gbs": round(alg * ((nq + 63) // 64) / t_scan / 1e9, 1),
                            "note": "32 flop per corpus byte at 64 queries: 4.9 TB/s of HBM at the f32 MFMA peak"}
                emit({"metric": "doc-queries/sec cosine scan + top-10 (dim 384)", "value": round(n * nq / t_all, 0),
                      "unit": "doc-queries/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
                      "config": {"workload": f"corpus [{n}, 384] unit-norm Gaussian rows resident in HBM, {nq} quer{'y' if nq == 1 else 'ies'}, k=10"},
                      "topk_set_equals_torch_topk": same, "ms_scan": round(t_scan * 1e3, 4), "ms_topk": round(t_topk * 1e3, 4),
                      "ms_total": round(t_all * 1e3, 4), "ms_search_one_call": round(t_search * 1e3, 4),
                      "search_gbs": round(alg * ((nq + 3) // 4 if nq < 20 else (nq + 63) // 64) / t_search / 1e9, 1),
                      "one_call_equals_two_calls_bit_for_bit": fused_equal, "roofline": roof})
                del scores, ws, idx, sc, q
            del corpus
            torch.cuda.empty_cache()

    if "strings" in which:
        rng = np.random.default_rng(0)
        vocab = json.load(open(os.path.join(emb_dir, "tokenizer.json")))["model"]["vocab"]
        words = [w for w in vocab if w.isalpha() and len(w) > 2][:4000] or ["alpha", "beta", "gamma"]
        n = 65536
        texts = [" ".join(rng.choice(words, 100)) for _ in range(n)]
        emb = kjarni_amd.Embedder("minilm-l6-v2", cache_dir=os.path.join(tmp, "cache"))
        emb.encode_batch(texts[:1024])
        t0 = time.perf_counter()
        out = emb.encode_batch(texts)
        dt = time.perf_counter() - t0
        tok = kjarni_amd.Tokenizer(os.path.join(emb_dir, "tokenizer.json"), 512)
        t0 = time.perf_counter()
        ids, mask, _ = tok.encode_batch(texts)
        dt_tok = time.perf_counter() - t0
        emit({"metric": "sentences/sec kjarni_embedder_encode_batch (strings in, host tokenisation included)",
              "value": round(n / dt, 1), "unit": "sentences/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
              "config": {"workload": f"{n} generated 100-word ASCII sentences, padded length {ids.shape[1]}"},
              "tokenise_only_sentences_per_s": round(n / dt_tok, 1), "host_threads": os.cpu_count(), "rows": int(out.shape[0])})
        # real text is ragged: the same handle on sentences of 8 .. 100 words (BatchLongest pads the call to the longest,
        # pipeline/encoder/loader.rs:98-115; the layers run over the kept tokens only)
        texts = [" ".join(rng.choice(words, int(rng.integers(8, 101)))) for _ in range(n)]
        emb.encode_batch(texts[:1024])
        t0 = time.perf_counter()
        out = emb.encode_batch(texts)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        ids, mask, _ = tok.encode_batch(texts)
        dt_tok = time.perf_counter() - t0
        emit({"metric": "sentences/sec kjarni_embedder_encode_batch (ragged strings in, host tokenisation included)",
              "value": round(n / dt, 1), "unit": "sentences/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
              "config": {"workload": f"{n} generated ASCII sentences of 8 .. 100 words, padded length {ids.shape[1]}, "
                                     f"kept tokens {float(mask.sum()) / mask.size:.3f} of the padded"},
              "tokenise_only_sentences_per_s": round(n / dt_tok, 1), "host_threads": os.cpu_count(), "rows": int(out.shape[0])})
        del emb

    if "latency" in which:
        # BASELINE.json configs[0] is a single-sentence classify; the reference serves it on the calling thread
        # (kjarni-ffi/src/lib.rs:25-32).  Per-call latency of the string-level entry points for ONE ~16-token sentence
        # (tokenise + H2D + forward + D2H + result shaping), single caller and four concurrent callers on one handle.
        import threading
        cls_dir = os.path.join(tmp, "cache", "distilbert_distilbert-base-uncased-finetuned-sst-2-english")
        synth.distilbert_sentiment(cls_dir, seed=2, n_layers=6, dim=768, n_heads=12, hidden_dim=3072)
        synth.add_tokenizer(cls_dir)
        sentence = "the quick brown fox jumps over the lazy dog near the old river bank today"
        emb = kjarni_amd.Embedder("minilm-l6-v2", cache_dir=os.path.join(tmp, "cache"))
        clf = kjarni_amd.Classifier(model_path=cls_dir)
        tok = kjarni_amd.Tokenizer(os.path.join(emb_dir, "tokenizer.json"), 512)
        n_tok = int(tok.encode_batch([sentence])[0].shape[1])

        def lat(fn, n=400, warm=30):
            for _ in range(warm):
                fn()
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            return {"p50_ms": round(ts[len(ts) // 2], 4), "p99_ms": round(ts[int(len(ts) * 0.99)], 4), "min_ms": round(ts[0], 4)}

        def concurrent(fn, threads=4, n=200):
            res = [None] * threads

            def run(i):
                res[i] = lat(fn, n=n, warm=10)
            th = [threading.Thread(target=run, args=(i,)) for i in range(threads)]
            t0 = time.perf_counter()
            for t in th:
                t.start()
            for t in th:
                t.join()
            wall = time.perf_counter() - t0
            return {"threads": threads, "calls_per_s": round(threads * (n + 10) / wall, 1),
                    "p50_ms": round(float(np.median([r["p50_ms"] for r in res])), 4),
                    "p99_ms": round(max(r["p99_ms"] for r in res), 4)}

        emit({"metric": "latency of one sentence through the string-level C ABI", "unit": "ms", "tokens": n_tok, "n_gpus": 1,
              "dtype": "f32", "data": "synthetic",
              "kjarni_embedder_encode (minilm-l6-v2 shape)": lat(lambda: emb.encode(sentence)),
              "kjarni_classifier_classify (distilbert-sst2 shape, 6 x 768)": lat(lambda: clf.classify(sentence)),
              "kjarni_embedder_encode, 4 threads on one handle": concurrent(lambda: emb.encode(sentence)),
              "kjarni_embedder_encode, 16 threads on one handle": concurrent(lambda: emb.encode(sentence), threads=16),
              "kjarni_classifier_classify, 4 threads on one handle": concurrent(lambda: clf.classify(sentence)),
              "kjarni_classifier_classify, 16 threads on one handle": concurrent(lambda: clf.classify(sentence), threads=16),
              "combining": os.environ.get("KJARNI_HIP_COMBINE", "0") not in ("", "0"),
              "note": "with KJARNI_HIP_COMBINE=1 small calls that arrive while another is on the device are combined into one "
                      "packed forward (kjarni_hip_encoder_set_combining: opt-in, default off)"})
        del emb, clf

    if "indexer" in which:
        rng = np.random.default_rng(0)
        words = ["alpha", "beta", "gamma", "delta", "kernel", "vector", "index", "search", "wave", "matrix", "iceland", "river"]
        docs = os.path.join(tmp, "docs")
        os.makedirs(docs)
        for i in range(400):
            paras = [" ".join(rng.choice(words, int(rng.integers(20, 80)))) + "." for _ in range(40)]
            with open(os.path.join(docs, f"doc{i:04d}.txt"), "w") as f:
                f.write("\n\n".join(paras))
        ix = kjarni_amd.Indexer(cache_dir=os.path.join(tmp, "cache"), quiet=True)
        ix.create(os.path.join(tmp, "warm"), [os.path.join(docs, "doc0000.txt")])
        t0 = time.perf_counter()
        st = ix.create(os.path.join(tmp, "index"), [docs])
        dt = time.perf_counter() - t0
        emit({"metric": "chunks/sec kjarni_indexer_create (files -> chunks -> embeddings -> segments on disk)",
              "value": round(st.documents_indexed / dt, 1), "unit": "chunks/s", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
              "config": {"workload": f"400 generated text files, chunk_size 512 / overlap 50 / batch_size 32 (defaults): "
                                     f"{st.documents_indexed} chunks, index {st.size_bytes} bytes"},
              "elapsed_ms": st.elapsed_ms})

    if "search" in which:
        # End-to-end retrieval over an on-disk index in the reference's segmented layout: 200 000 documents in 20 segments of
        # 10 000 (the default max_docs_per_segment), dim 384; every query re-opens the index as Searcher::search does, the
        # segments' vectors stay resident in HBM between queries.
        from kjarni_amd.indexer import index_write
        from kjarni_amd.searcher import index_search, search_keywords
        rng = np.random.default_rng(3)
        n_docs, dim = 200_000, 384
        words = ["alpha", "beta", "gamma", "delta", "kernel", "vector", "index", "search", "wave", "matrix", "iceland", "river", "glacier",
                 "basalt", "harbour", "northern", "lights", "wool", "fjord", "geyser"]
        ipath = os.path.join(tmp, "big_index")
        t0 = time.perf_counter()
        for start in range(0, n_docs, 50_000):
            texts = [" ".join(rng.choice(words, 12)) + f" doc{start + i}" for i in range(50_000)]
            emb = rng.standard_normal((50_000, dim), dtype=np.float32)
            index_write(ipath, dim, texts, emb, [{"source": f"f{(start + i) % 97}.txt"} for i in range(50_000)], append=start > 0)
        t_build = time.perf_counter() - t0
        queries = rng.standard_normal((64, dim), dtype=np.float32)
        index_search(ipath, None, queries[0], mode="semantic", top_k=10)      # first query uploads the segments
        runs = {}
        for label, fn in (("semantic", lambda q: index_search(ipath, None, q, mode="semantic", top_k=10)),
                          ("keyword", lambda q: search_keywords(ipath, "glacier fjord basalt", 10)),
                          ("hybrid", lambda q: index_search(ipath, "glacier fjord basalt", q, mode="hybrid", top_k=10)),
                          ("semantic_filtered", lambda q: index_search(ipath, None, q, mode="semantic", top_k=10, source_pattern="f1*.txt"))):
            fn(queries[1])
            from kjarni_amd.searcher import search_breakdown
            t0 = time.perf_counter()
            acc = {}
            for q in queries[:32]:
                r = fn(q)
                for k_, v_ in search_breakdown().items():
                    acc[k_] = acc.get(k_, 0.0) + v_ / 32
            dt = (time.perf_counter() - t0) / 32
            # per query, microseconds: re-opening the index | the scan over the device image (of it the device round trip) | the
            # rest on the host (BM25, fusion, reading the hits' documents and metadata back)
            runs[label] = {"ms_per_query": round(dt * 1e3, 3), "queries_per_s": round(1.0 / dt, 1), "results": len(r),
                           "breakdown_us": {k_: round(v_, 1) for k_, v_ in acc.items()}}
        # the whole Searcher: query string -> tokenise -> embed on the GPU -> retrieval (-> cross-encoder over 5x candidates)
        ce_dir = os.path.join(tmp, "cache", "cross-encoder_ms-marco-MiniLM-L-6-v2")
        synth.minilm_cross_encoder(ce_dir, seed=1)
        synth.add_tokenizer(ce_dir)
        for label, kw in (("searcher_semantic", dict(mode="semantic")), ("searcher_hybrid", dict(mode="hybrid")),
                          ("searcher_hybrid_rerank", dict(mode="hybrid", rerank=True))):
            sr = kjarni_amd.Searcher("minilm-l6-v2", "minilm-l6-v2-cross-encoder" if "rerank" in label else None, device="gpu",
                                     cache_dir=os.path.join(tmp, "cache"))
            qs = [" ".join(rng.choice(words, 6)) for _ in range(33)]
            sr.search(ipath, qs[0], top_k=10, **kw)
            t0 = time.perf_counter()
            for q in qs[1:]:
                r = sr.search(ipath, q, top_k=10, **kw)
            dt = (time.perf_counter() - t0) / 32
            runs[label] = {"ms_per_query": round(dt * 1e3, 3), "queries_per_s": round(1.0 / dt, 1), "results": len(r)}
            del sr
        emit({"metric": "ms per query, retrieval over an on-disk index (200 000 docs x 384, 20 segments), top-10", "unit": "ms",
              "value": runs["semantic"]["ms_per_query"], "higher_is_better": False, "n_gpus": 1, "dtype": "f32", "data": "synthetic",
              "config": {"workload": "kjarni_hip_index_search / kjarni_search_keywords on an index written by kjarni_index_write; "
                                     "documents and metadata are read back from docs.bin / metadata.jsonl for the 10 hits"},
              "index_build_seconds": round(t_build, 2), "runs": runs})

    if "whisper" in which:
        d = os.path.join(tmp, "whisper-base")
        cfg_w, t_w = synth.whisper_model(d, seed=0, base=True)
        wm = kjarni_amd.HipWhisper(d)
        audio = synth.synthetic_audio(30.0, seed=1)
        n_tok = 448
        prompt = [50258, 50259, 50359, 50363]
        wm.encode_audio(audio, fetch=False)
        wm.greedy(prompt, False, 8)                                   # warm-up
        t_mel = timed(lambda: wm.log_mel(audio), lambda: None, 5, 1)  # includes the D2H of the mel
        t_enc = timed(lambda: wm.encode_audio(audio, fetch=False), lambda: None, 5, 1)   # mel + stem + encoder, synchronised
        t0 = time.perf_counter()
        ids = wm.greedy(prompt, False, n_tok)
        t_dec = time.perf_counter() - t0
        total = t_enc + t_dec
        H, L_, I, S_, V = 512, 6, 2048, 1500, 51865
        enc_flops = L_ * (2 * S_ * H * 3 * H + 4 * S_ * S_ * H + 2 * S_ * H * H + 4 * S_ * H * I) + 2 * 3000 * 512 * 240 + 2 * 1500 * 512 * 1536
        # decoder step: weights streamed once per token (HBM-bound): 6 layers x (8 HxH + 2 HxI) + lm head, + cross K/V reads
        dec_bytes = 4 * (L_ * (8 * H * H + 2 * H * I) + V * H + L_ * 2 * S_ * H)
        res = {"metric": "x real time, Whisper-base shaped transcribe of 30 s audio (log-mel + encoder + greedy decode)",
               "value": round(30.0 / total, 1), "unit": "x real time", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "BASELINE.json configs[3]: whisper-base shape (d=512, 6+6 layers, vocab 51865), random init, "
                                      f"30 s synthetic audio, {len(ids)} generated tokens (EOS is never the argmax with random weights)"},
               "ms_log_mel_incl_d2h": round(t_mel * 1e3, 3), "ms_mel_stem_encoder": round(t_enc * 1e3, 3),
               "ms_decode": round(t_dec * 1e3, 2), "ms_per_token": round(t_dec * 1e3 / len(ids), 4),
               "tokens_per_s": round(len(ids) / t_dec, 1),
               "encoder_tflops": round(enc_flops / t_enc / 1e12, 2),
               "decode_weight_stream_gbs": round(dec_bytes * len(ids) / t_dec / 1e9, 1),
               "decode_frac_hbm_peak": round(dec_bytes * len(ids) / t_dec / 1e9 / PEAK_HBM_GBS, 4)}
        # CPU restatement (oracle): one encoder pass + a few decoder steps, extrapolated to the same token count
        from oracle import whisper_oracle as WO
        cores = usable_cores()
        from oracle import oracle as O
        O.lib().ko_set_num_threads(int(cores))
        orc = WO.WhisperOracle(t_w, cfg_w)
        t0 = time.perf_counter()
        mel = WO.log_mel(audio)
        c_mel = time.perf_counter() - t0
        t0 = time.perf_counter()
        enc = orc.encode_mel(mel)
        c_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        orc.decode_chunk_ids(enc, max_tokens=15)
        c_dec16 = time.perf_counter() - t0
        c_total = c_mel + c_enc + c_dec16 / 16 * len(ids)
        res["cpu_baseline"] = {"value": round(30.0 / c_total, 3), "unit": "x real time", "cores": int(cores), "kind": "port",
                               "sample": f"oracle: log-mel {c_mel:.2f} s (vectorised DFT, not the reference's scalar O(n^2) loop), "
                                         f"encoder {c_enc:.2f} s, 16 decoder steps {c_dec16:.2f} s extrapolated to {len(ids)} tokens"}
        emit(res)
        # A long recording through the string-level Transcriber: 16 chunks of 30 s (8 minutes), 448 tokens per chunk,
        # chunk by chunk vs eight chunks per decoder launch (the default without a per-token callback).
        tr = kjarni_amd.Transcriber(model_path=d, max_tokens=n_tok)
        long_audio = np.concatenate([synth.synthetic_audio(30.0, seed=20 + i) for i in range(16)])
        tr.transcribe_audio(long_audio[: 16000 * 45], 16000)          # warm-up (graphs for 2 lanes do not matter below)
        rows = {}
        for label, lanes in (("sequential", "1"), ("lock_step_8", "8")):
            os.environ["KJARNI_HIP_WHISPER_LANES"] = lanes
            tr.transcribe_audio(long_audio, 16000)
            t0 = time.perf_counter()
            out = tr.transcribe_audio(long_audio, 16000)
            dt = time.perf_counter() - t0
            rows[label] = {"seconds": round(dt, 3), "x_real_time": round(480.0 / dt, 1), "chars": len(out.text)}
        os.environ.pop("KJARNI_HIP_WHISPER_LANES", None)
        emit({"metric": "x real time, Whisper-base shaped transcribe of 8 min audio (16 chunks x 448 tokens) through kjarni_transcriber_*",
              "value": rows["lock_step_8"]["x_real_time"], "unit": "x real time", "n_gpus": 1, "dtype": "f32", "data": "synthetic",
              "config": {"workload": "whisper-base shape, random init, 480 s synthetic audio, 449 generated tokens per chunk"},
              "runs": rows, "same_text": rows["sequential"]["chars"] == rows["lock_step_8"]["chars"]})

    if "gpt2" in which:
        # gpt2-small shape (768 hidden, 12 layers, 12 heads, 3 072 MLP, vocab 50 257, n_ctx 1 024), random weights: bf16 stored,
        # then the same weights as f32; 128-token prompt, 256 greedy tokens (no eos: every token is generated)
        from tests import gpt2_fixture
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        prompt = np.random.default_rng(0).integers(0, 50257, 128).tolist()
        n_new = 256
        bf16_row = None
        for weights in ("auto", "f32"):
            dec = kjarni_amd.HipDecoder(gd, weights=weights)
            dec.generate(prompt, 8)                                           # warm-up (graph capture)
            t0 = time.perf_counter()
            dec.reset()
            dec.forward(prompt, fetch=False)
            t_prefill = time.perf_counter() - t0
            t0 = time.perf_counter()
            out = dec.generate(prompt, n_new)
            t_dec = time.perf_counter() - t0 - t_prefill
            kv_bytes = 2 * 12 * 768 * 4 * (128 + n_new / 2)                   # average cache read per step
            per_tok = dec.weight_bytes + kv_bytes
            row = {"metric": f"tokens/sec greedy decode, gpt2-small shape, {'bf16' if dec.bf16 else 'f32'} weights, batch 1",
                   "value": round(len(out) / t_dec, 1), "unit": "tokens/s", "n_gpus": 1,
                   "dtype": f"{'bf16' if dec.bf16 else 'f32'} weights, f32 activations/accumulate/KV", "data": "synthetic",
                   "config": {"workload": "gpt2-small geometry (768 hidden, 12 layers, 12 heads, 3 072 MLP, vocab 50 257, n_ctx 1 024), "
                                          f"random init, 128-token prompt, {len(out)} generated tokens"},
                   "ms_prefill_128": round(t_prefill * 1e3, 2), "ms_per_token": round(t_dec * 1e3 / len(out), 4),
                   "weight_bytes": dec.weight_bytes,
                   "roofline": {"kernel": "llm_gemv1 / llm_gemv_splitk (LayerNorm, GELU-tanh, residual) + decode_attention_partial",
                                "bound": "hbm", "achieved": round(per_tok * len(out) / t_dec / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                "frac": round(per_tok * len(out) / t_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                                "algorithmic_bytes_per_token": int(per_tok)},
                   "note": "the bf16 weights (about 249 MB) are close to the 256 MiB Infinity Cache, so part of the weight stream "
                           "may be served on-die and the HBM fraction overstates what HBM delivered"}
            if bf16_row is not None:
                row["bf16_same_run"] = {"tokens_per_s": bf16_row["value"], "ms_per_token": bf16_row["ms_per_token"]}
            else:
                bf16_row = row
            emit(row)
            del dec

    if "llm" in which:
        d = os.path.join(tmp, "llama-1b")
        cfg_l, t_l = synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        prompt = np.random.default_rng(0).integers(1000, 100000, 128).tolist()
        n_new = 256
        dec.generate(prompt, 8)                                               # warm-up (graph capture)
        t0 = time.perf_counter()
        dec.reset()
        dec.forward(prompt, fetch=False)
        t_prefill = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = dec.generate(prompt, n_new)
        t_total = time.perf_counter() - t0
        t_dec = t_total - t_prefill
        kv_dim = cfg_l["num_key_value_heads"] * 64
        kv_bytes = 2 * cfg_l["num_hidden_layers"] * kv_dim * 4 * (128 + n_new / 2)   # average cache read per step
        per_tok = dec.weight_bytes + kv_bytes
        res = {"metric": "tokens/sec greedy decode, Llama-3.2-1B shape, bf16 weights, batch 1", "value": round(len(out) / t_dec, 1),
               "unit": "tokens/s", "n_gpus": 1, "dtype": "bf16 weights, f32 activations/accumulate/KV", "data": "synthetic",
               "config": {"workload": "BASELINE.json configs[4]: Llama-3.2-1B geometry (2048 hidden, 16 layers, 32/8 heads, vocab 128256), "
                                      f"random init, 128-token prompt, {len(out)} generated tokens"},
               "ms_prefill_128": round(t_prefill * 1e3, 2), "prefill_tokens_per_s": round(128 / t_prefill, 1),
               "ms_per_token": round(t_dec * 1e3 / len(out), 4), "weight_bytes": dec.weight_bytes,
               "roofline": {"kernel": "llm_gemv_stream_kernel (weight stream) + decode_attention_partial", "bound": "hbm",
                            "achieved": round(per_tok * len(out) / t_dec / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                            "frac": round(per_tok * len(out) / t_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                            "algorithmic_bytes_per_token": int(per_tok)}}
        if not os.environ.get("KJARNI_BENCH_NO_CPU"):                         # kernel A/B runs skip the CPU leg
            from oracle import llm_oracle as LO
            from oracle import oracle as O
            cores = usable_cores()
            O.lib().ko_set_num_threads(int(cores))
            orc = LO.LlmOracle(t_l, cfg_l)
            cache = orc.new_cache()
            t0 = time.perf_counter()
            h = orc.forward(prompt[:16], cache)
            c_pre = time.perf_counter() - t0
            t0 = time.perf_counter()
            for i in range(4):
                h = orc.forward([int(out[i])], cache)
                orc.logits(h[0, -1])
            c_dec = (time.perf_counter() - t0) / 4
            res["cpu_baseline"] = {"value": round(1.0 / c_dec, 2), "unit": "tokens/s", "cores": int(cores), "kind": "port",
                                   "sample": f"oracle: 16-token prefill {c_pre:.2f} s, 4 decode steps at {c_dec * 1e3:.0f} ms each (f32 weights)"}
        emit(res)
        # The same geometry as a GGUF Q4_K_M-style mix (tests/gguf_fixture.py): Q6_K token_embd (the tied head) and Q6_K
        # attn_v / ffn_down in the even layers (0, 2, ..., 14), Q4_K everywhere else, F32 norms; matrices quantized in HBM.
        from tests import gguf_fixture
        gpath = os.path.join(tmp, "llama-1b-q4km.gguf")
        gcfg = dict(synth.LLAMA_1B, max_position_embeddings=4096, eos_token_id=cfg_l["vocab_size"] + 1)
        gguf_fixture.gguf_model(gpath, gcfg, gguf_fixture.q4_k_m_types(gcfg["num_hidden_layers"]), seed=0, rope_freqs=True, keep_hf=False)
        qdec = kjarni_amd.HipDecoder(gpath, max_context=2048)
        qdec.generate(prompt, 8)
        t0 = time.perf_counter()
        qdec.reset()
        qdec.forward(prompt, fetch=False)
        q_prefill = time.perf_counter() - t0
        t0 = time.perf_counter()
        qout = qdec.generate(prompt, n_new)
        q_dec = time.perf_counter() - t0 - q_prefill
        q_tok = qdec.weight_bytes + kv_bytes
        emit({"metric": "tokens/sec greedy decode, Llama-3.2-1B shape, GGUF Q4_K_M mix in HBM, batch 1", "value": round(len(qout) / q_dec, 1),
              "unit": "tokens/s", "n_gpus": 1, "dtype": "Q4_K / Q6_K weights, f32 activations/accumulate/KV", "data": "synthetic",
              "config": {"workload": "Llama-3.2-1B geometry as GGUF: Q6_K token_embd (tied head) and attn_v / ffn_down of layers 0, 2, ..., 14, "
                                     f"Q4_K elsewhere, F32 norms; random blocks, 128-token prompt, {len(qout)} generated tokens"},
              "ms_prefill_128": round(q_prefill * 1e3, 2), "ms_per_token": round(q_dec * 1e3 / len(qout), 4),
              "weight_bytes": qdec.weight_bytes, "weight_bytes_by_type": qdec.weight_bytes_by_type(),
              "bf16_same_run": {"tokens_per_s": res["value"], "ms_per_token": res["ms_per_token"], "weight_bytes": dec.weight_bytes},
              "speedup_vs_bf16": round((len(qout) / q_dec) / res["value"], 3),
              "weight_bytes_ratio_vs_bf16": round(qdec.weight_bytes / dec.weight_bytes, 3),
              "roofline": {"kernel": "qfused_kernel (weight stream) + decode_attention_partial", "bound": "hbm",
                           "achieved": round(q_tok * len(qout) / q_dec / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                           "frac": round(q_tok * len(qout) / q_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                           "algorithmic_bytes_per_token": int(q_tok)}})
        del qdec
        # FP8 (e4m3) checkpoints, the codes kept in HBM (tests/fp8_fixture.py): the Llama-1B shape with per-channel scales beside
        # the bf16 entry above, and the Qwen3-0.6B shape with 128 x 128 block scales beside a bf16 load of the same shape.
        from tests import fp8_fixture, qwen3_fixture

        def decode_run(d8):
            d8.generate(prompt, 8)                                            # warm-up (graph capture)
            t0 = time.perf_counter()
            d8.reset()
            d8.forward(prompt, fetch=False)
            pre = time.perf_counter() - t0
            t0 = time.perf_counter()
            o = d8.generate(prompt, n_new)
            return pre, time.perf_counter() - t0 - pre, len(o)

        def fp8_entry(label, fdec, base, kvb, what):
            f_pre, f_dec, f_n = decode_run(fdec)
            table = fdec.weight_bytes_by_type().get("BF16", 0)                # one row of the table is read; the tied head streams it
            f_tok = fdec.weight_bytes + kvb
            emit({"metric": f"tokens/sec greedy decode, {label}, FP8 e4m3 weights in HBM, batch 1", "value": round(f_n / f_dec, 1),
                  "unit": "tokens/s", "n_gpus": 1, "dtype": "F8_E4M3 layer weights + f32 scales, bf16 table / head, f32 activations/accumulate/KV",
                  "data": "synthetic", "config": {"workload": f"{what}; random codes, 128-token prompt, {f_n} generated tokens"},
                  "ms_prefill_128": round(f_pre * 1e3, 2), "ms_per_token": round(f_dec * 1e3 / f_n, 4),
                  "weight_bytes": fdec.weight_bytes, "weight_bytes_by_type": fdec.weight_bytes_by_type(), "table_bytes": table,
                  "bf16_same_run": base, "speedup_vs_bf16": round((f_n / f_dec) / base["tokens_per_s"], 3),
                  "prefill_ratio_vs_bf16": round(f_pre * 1e3 / base["ms_prefill_128"], 3),
                  "weight_bytes_ratio_vs_bf16": round(fdec.weight_bytes / base["weight_bytes"], 3),
                  "roofline": {"kernel": "fp8_proj_kernel (weight stream) + decode_attention_partial", "bound": "hbm",
                               "achieved": round(f_tok * f_n / f_dec / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                               "frac": round(f_tok * f_n / f_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                               "algorithmic_bytes_per_token": int(f_tok)}})

        fdir = os.path.join(tmp, "llama-1b-fp8")
        fcfg = dict(synth.LLAMA_1B, max_position_embeddings=4096, eos_token_id=cfg_l["vocab_size"] + 1)
        fp8_fixture.fp8_model(fdir, fcfg, "channel", seed=0, keep_hf=False)
        fdec = kjarni_amd.HipDecoder(fdir, max_context=2048)
        fp8_entry("Llama-3.2-1B shape", fdec, {"tokens_per_s": res["value"], "ms_per_token": res["ms_per_token"],
                                                "ms_prefill_128": res["ms_prefill_128"], "weight_bytes": dec.weight_bytes}, kv_bytes,
                  "Llama-3.2-1B geometry, the seven matrices of every layer F8_E4M3 with per-channel scales")
        del fdec
        q3 = dict(fp8_fixture.QWEN3_06B, max_position_embeddings=4096, eos_token_id=fp8_fixture.QWEN3_06B["vocab_size"] + 1)
        bdir = os.path.join(tmp, "qwen3-06b-bf16")
        qwen3_fixture.qwen3_model(bdir, q3, seed=0, store_bf16=True)
        bdec = kjarni_amd.HipDecoder(bdir, max_context=2048)
        b_pre, b_dec, b_n = decode_run(bdec)
        base = {"tokens_per_s": round(b_n / b_dec, 1), "ms_per_token": round(b_dec * 1e3 / b_n, 4), "ms_prefill_128": round(b_pre * 1e3, 2),
                "weight_bytes": bdec.weight_bytes}
        del bdec
        fdir = os.path.join(tmp, "qwen3-06b-fp8")
        fp8_fixture.fp8_model(fdir, q3, "block", seed=0, keep_hf=False)
        fdec = kjarni_amd.HipDecoder(fdir, max_context=2048)
        q3_kv = 2 * q3["num_hidden_layers"] * q3["num_key_value_heads"] * q3["head_dim"] * 4 * (128 + n_new / 2)
        fp8_entry("Qwen3-0.6B shape", fdec, base, q3_kv,
                  "Qwen3-0.6B geometry (hidden 1024, 28 layers, 16/8 heads of 128, inter 3072, vocab 151936, tied head), the seven matrices "
                  "of every layer F8_E4M3 with 128 x 128 block scales")
        del fdec

    if "llm8b" in which:
        # The same decode path on the Llama-3.1-8B geometry (16 GB of bf16 weights): the per-kernel floor that bounds the 1B
        # shape is amortised over 6.5x more bytes per launch, so this shows what the weight-streaming kernels reach.
        d = os.path.join(tmp, "llama-8b")
        cfg_l = synth.llm_model_streamed(d, synth.LLAMA_8B, seed=0, max_position_embeddings=4096, eos_token_id=[])
        t0 = time.perf_counter()
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        t_load = time.perf_counter() - t0
        prompt = np.random.default_rng(0).integers(1000, 100000, 512).tolist()
        n_new = 128
        dec.generate(prompt[:32], 8)
        dec.reset()
        dec.forward(prompt, fetch=False)
        t0 = time.perf_counter()
        dec.reset()
        dec.forward(prompt, fetch=False)
        t_prefill = time.perf_counter() - t0
        t0 = time.perf_counter()
        out = dec.generate(prompt, n_new)
        t_dec = time.perf_counter() - t0 - t_prefill
        kv_bytes = 2 * cfg_l["num_hidden_layers"] * cfg_l["num_key_value_heads"] * 128 * 4 * (512 + n_new / 2)
        per_tok = dec.weight_bytes - 128256 * 4096 * 2 + kv_bytes   # the embedding table is not streamed (one row is read)
        flops_prefill = 2.0 * 512 * (dec.weight_bytes / 2 - 2 * 128256 * 4096)
        emit({"metric": "tokens/sec greedy decode, Llama-3.1-8B shape, bf16 weights, batch 1", "value": round(len(out) / t_dec, 1),
              "unit": "tokens/s", "n_gpus": 1, "dtype": "bf16 weights, f32 activations/accumulate/KV", "data": "synthetic",
              "config": {"workload": "Llama-3.1-8B geometry (4096 hidden, 32 layers, 32/8 heads of 128, inter 14336, vocab 128256, untied head), "
                                     f"random init, 512-token prompt, {len(out)} generated tokens"},
              "ms_per_token": round(t_dec * 1e3 / len(out), 4), "ms_prefill_512": round(t_prefill * 1e3, 2),
              "prefill_tokens_per_s": round(512 / t_prefill, 1), "prefill_tflops": round(flops_prefill / t_prefill / 1e12, 1),
              "weight_bytes": dec.weight_bytes, "load_seconds": round(t_load, 1),
              "roofline": {"kernel": "llm_gemv_splitk_kernel (weight stream)", "bound": "hbm", "achieved": round(per_tok * len(out) / t_dec / 1e9, 1),
                           "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(per_tok * len(out) / t_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                           "algorithmic_bytes_per_token": int(per_tok)}})

    if "chat" in which:
        # The string-level path of the C ABI (kjarni_chat_send / kjarni_chat_stream) on the same Llama-1B shape: template,
        # BPE encode, prefill, decode with the sampler, per-token text.  The tokenizer is the small Llama-3-style fixture
        # (the model's 128 256-row head is kept, so the sampler sees a full-size vocabulary).
        import shutil
        from kjarni_amd.chat import Chat, GenerationConfig
        d = os.path.join(tmp, "llama-1b-chat")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, bos_token_id=700, eos_token_id=[701])
        shutil.copy(os.path.join(ROOT, "tests", "golden", "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
        chat = Chat("llama3.2-1b-instruct", model_path=d)
        message = "Summarise the history of Iceland in three paragraphs, please. " * 4
        n_prompt = len(chat.encode(chat.format_prompt(None, message)))
        n_new = 256
        rows = {}
        for label, g in [("greedy", GenerationConfig(do_sample=False, max_new_tokens=n_new)),
                         ("sample_default", GenerationConfig(max_new_tokens=n_new)),
                         ("sample_top_k40_rep1.1", GenerationConfig(max_new_tokens=n_new, top_k=40, repetition_penalty=1.1))]:
            chat.seed(1)
            chat.send(message, GenerationConfig(do_sample=g.do_sample, max_new_tokens=8))   # warm-up
            pieces = []
            first = []
            t0 = time.perf_counter()

            def on_token(text, pieces=pieces, first=first, t0=t0):
                if not pieces:
                    first.append(time.perf_counter() - t0)
                pieces.append(text)
                return True

            chat.stream(message, on_token, g)
            dt = time.perf_counter() - t0
            rows[label] = {"tokens": len(pieces), "ms_to_first_token": round(first[0] * 1e3, 2) if first else None,
                           "tokens_per_s_after_first": round((len(pieces) - 1) / (dt - first[0]), 1) if len(pieces) > 1 else None,
                           "ms_total": round(dt * 1e3, 1)}
        # Random weights give a nearly flat next-token distribution (top-p 0.9 keeps thousands of tokens: the sampler's worst
        # case).  A trained model's is peaked; the same checkpoint with its final norm scaled 8x stands in for that.
        from safetensors.torch import load_file, save_file
        d2 = os.path.join(tmp, "llama-1b-chat-peaked")
        os.makedirs(d2)
        for name in ("config.json", "tokenizer.json"):
            shutil.copy(os.path.join(d, name), os.path.join(d2, name))
        tensors = load_file(os.path.join(d, "model.safetensors"))
        tensors["model.norm.weight"] = tensors["model.norm.weight"] * 8.0
        save_file(tensors, os.path.join(d2, "model.safetensors"))
        del tensors
        chat2 = Chat("llama3.2-1b-instruct", model_path=d2)
        chat2.seed(1)
        chat2.send(message, GenerationConfig(max_new_tokens=8))
        pieces, first = [], []
        t0 = time.perf_counter()

        def on_token2(text):
            if not pieces:
                first.append(time.perf_counter() - t0)
            pieces.append(text)
            return True

        chat2.stream(message, on_token2, GenerationConfig(max_new_tokens=n_new))
        dt = time.perf_counter() - t0
        rows["sample_default_peaked_logits"] = {"tokens": len(pieces), "ms_to_first_token": round(first[0] * 1e3, 2),
                                                "tokens_per_s_after_first": round((len(pieces) - 1) / (dt - first[0]), 1),
                                                "ms_total": round(dt * 1e3, 1)}
        del chat2
        t0 = time.perf_counter()
        for _ in range(20):
            chat.encode(chat.format_prompt(None, message))
        t_enc = (time.perf_counter() - t0) / 20
        emit({"metric": "chat tokens/sec through kjarni_chat_stream, Llama-3.2-1B shape, bf16 weights", "unit": "tokens/s",
              "value": rows["greedy"]["tokens_per_s_after_first"], "n_gpus": 1, "data": "synthetic",
              "config": {"workload": f"Llama-3.2-1B geometry, random init, {n_prompt}-token templated prompt, {n_new} new tokens; "
                                     "greedy = device-resident graph loop, sample = logits to the host + sampler per token"},
              "prompt_tokens": n_prompt, "ms_template_plus_bpe_encode": round(t_enc * 1e3, 3), "runs": rows})

    if "llm_lanes" in which:
        # Method (measuring guide, section 5): everything in one process on one box; every lane count is warmed first (graph
        # capture, lane caches); the decode window is a whole generation minus the same call cut after its first token (the
        # prefills and the first pick), so it holds n_new - 1 lock-step steps; lanes = 1 / 2 / 4 / 8 alternate with the
        # single-stream generate() -- the yardstick -- twice.
        from tests import gguf_fixture, gpt2_fixture
        rng = np.random.default_rng(0)
        trace_steps = int(os.environ.get("KJARNI_LANES_STEPS", "0"))

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, prompts, n_new, dtype):
            if trace_steps:  # a short run for rocprofv3 --kernel-trace --stats: 8 lanes, trace_steps lock-step steps
                dec.generate_batch(prompts, trace_steps + 1, lanes=8)
                return
            single_rates, rows = [], {}
            dec.generate(prompts[0], 8)
            for lanes in (1, 2, 4, 8):
                dec.generate_batch(prompts[:lanes], 20, lanes=lanes)               # warm-up: graph capture for this lane count
            for rep in range(2):
                for lanes in (1, 2, 4, 8):
                    dt, out = window(lambda: dec.generate(prompts[0], n_new), lambda: dec.generate(prompts[0], 1))
                    assert len(out) == n_new
                    single_rates.append((n_new - 1) / dt)
                    ps = prompts[:lanes]
                    dt, outs = window(lambda: dec.generate_batch(ps, n_new, lanes=lanes), lambda: dec.generate_batch(ps, 1, lanes=lanes))
                    assert all(len(o) == n_new for o in outs)
                    rows.setdefault(lanes, []).append({"tokens_per_s": round(lanes * (n_new - 1) / dt, 1),
                                                       "ms_per_step": round(dt * 1e3 / (n_new - 1), 4)})
            single = float(np.median(single_rates))
            emit({"metric": f"aggregate tokens/sec greedy decode in lanes, {label}", "unit": "tokens/s",
                  "value": max(r["tokens_per_s"] for r in rows[8]), "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                  "config": {"workload": f"{label}, random init, one 128-token prompt per lane, {n_new} generated tokens per lane, "
                                         "lanes 1 / 2 / 4 / 8 alternated twice with single-stream generate() in one process"},
                  "single_stream_tokens_per_s": {"median": round(single, 1), "min": round(min(single_rates), 1),
                                                 "max": round(max(single_rates), 1), "runs": [round(r, 1) for r in single_rates]},
                  "lanes": {str(k): v for k, v in rows.items()},
                  "x_single_stream_at_8": round(max(r["tokens_per_s"] for r in rows[8]) / single, 2), "weight_bytes": dec.weight_bytes})

        d = os.path.join(tmp, "llama-1b-lanes")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        prompts = [rng.integers(1000, 100000, 128).tolist() for _ in range(8)]
        measure("Llama-3.2-1B shape, bf16 weights", dec, prompts, 1024, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        if not trace_steps:  # (the trace run is the Llama shape alone)
            gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
            gd = os.path.join(tmp, "gpt2-small-lanes")
            gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
            gprompts = [rng.integers(0, 50257, 128).tolist() for _ in range(8)]
            for weights in ("auto", "f32"):
                dec = kjarni_amd.HipDecoder(gd, weights=weights)
                wt = "bf16" if dec.bf16 else "f32"
                measure(f"gpt2-small shape, {wt} weights", dec, gprompts, 768, f"{wt} weights, f32 activations/accumulate/KV")
                del dec
            gpath = os.path.join(tmp, "llama-1b-q4km-lanes.gguf")
            qcfg = dict(synth.LLAMA_1B, max_position_embeddings=4096, eos_token_id=synth.LLAMA_1B["vocab_size"] + 1)
            gguf_fixture.gguf_model(gpath, qcfg, gguf_fixture.q4_k_m_types(qcfg["num_hidden_layers"]), seed=0, rope_freqs=True, keep_hf=False)
            dec = kjarni_amd.HipDecoder(gpath, max_context=2048)
            measure("Llama-3.2-1B shape, GGUF Q4_K_M-style mix (Q4_K / Q6_K in HBM)", dec, prompts, 512, "Q4_K / Q6_K weights, f32 activations/KV")
            del dec

    if "llm_wide" in which:
        # Method (as llm_lanes): one process on one box; every leg is warmed first (graph capture, lane caches); a decode window is
        # a whole call minus the same call cut after its first token (the prefills and the first pick), so it holds n_new - 1
        # lock-step steps.  Legs, twice over: single-stream generate() and generate_batch at 8 lanes -- both code from before the
        # wide route, the baselines -- then generate_wide at 16 / 32 / 64 lanes.  One 128-token prompt per lane, 128 new tokens,
        # lane_context 512.
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        trace_steps = int(os.environ.get("KJARNI_WIDE_STEPS", "0"))
        n_new, ctx = 128, 512

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure_wide(label, dec, prompts, dtype):
            if trace_steps:  # a short run for rocprofv3 --kernel-trace --stats: 64 lanes, trace_steps wide steps
                dec.generate_wide(prompts, trace_steps + 1, lanes=64, lane_context=ctx)
                return
            legs = {"single": lambda n: [dec.generate(prompts[0], n)],
                    "lanes-8": lambda n: dec.generate_batch(prompts[:8], n, lanes=8, lane_context=ctx)}
            for w in (16, 32, 64):
                legs[f"wide-{w}"] = (lambda w: lambda n: dec.generate_wide(prompts[:w], n, lanes=w, lane_context=ctx))(w)
            width = {"single": 1, "lanes-8": 8, "wide-16": 16, "wide-32": 32, "wide-64": 64}
            for fn in legs.values():
                fn(20)
            rows = {}
            for rep in range(2):
                for name, fn in legs.items():
                    dt, outs = window(lambda: fn(n_new), lambda: fn(1))
                    assert all(len(o) == n_new for o in outs)
                    rows.setdefault(name, []).append({"tokens_per_s": round(width[name] * (n_new - 1) / dt, 1),
                                                      "ms_per_step": round(dt * 1e3 / (n_new - 1), 4)})
            best = {k: max(r["tokens_per_s"] for r in v) for k, v in rows.items()}
            emit({"metric": f"aggregate tokens/sec greedy decode in wide lanes, {label}", "unit": "tokens/s", "value": best["wide-64"],
                  "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                  "config": {"workload": f"{label}, random init, one 128-token prompt per lane, {n_new} generated tokens per lane, lane_context "
                                         f"{ctx}; generate(), generate_batch at 8 lanes, generate_wide at 16 / 32 / 64, twice, in one process"},
                  "legs": rows, "x_lanes_8": {k: round(best[k] / best["lanes-8"], 2) for k in ("wide-16", "wide-32", "wide-64")},
                  "x_single_stream": {k: round(best[k] / best["single"], 2) for k in best if k != "single"}, "weight_bytes": dec.weight_bytes})

        d = os.path.join(tmp, "llama-1b-wide")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        prompts = [rng.integers(1000, 100000, 128).tolist() for _ in range(64)]
        measure_wide("Llama-3.2-1B shape, bf16 weights", dec, prompts, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        if not trace_steps:  # (the trace run is the Llama shape alone)
            gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
            gd = os.path.join(tmp, "gpt2-small-wide")
            gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
            gprompts = [rng.integers(0, 50257, 128).tolist() for _ in range(64)]
            dec = kjarni_amd.HipDecoder(gd)
            measure_wide("gpt2-small shape, bf16 weights", dec, gprompts, "bf16 weights, f32 activations/accumulate/KV")
            del dec

    if "llm_wide_fp8" in which:
        # FP8 checkpoints on the matrix cores (HipDecoder.set_fp8_matrix_cores).  Method (as llm_wide): one process on one box, every
        # leg warmed first, every leg twice, best of two; a decode window is a whole call minus the same call cut after its first
        # token.  Per shape -- Llama-3.2-1B with per-channel scales, Qwen3-0.6B with 128 x 128 block scales, random codes of
        # tests/fp8_fixture.py -- FP8 generate_batch at 8 lanes (the switch off: all an FP8 checkpoint could do before), FP8
        # generate_wide at 16 / 32 / 64 with the switch on, a bf16 load of the same shape at the same widths; and the prompt's
        # time at 128 and 384 tokens with the switch off, on, and for bf16 (median of 5 forward() calls that end in a synchronise).
        from tests import fp8_fixture, qwen3_fixture
        rng = np.random.default_rng(0)
        n_new, ctx = 64, 512
        out_path = os.path.join(ROOT, "profiles", "llm_wide_fp8_bench.jsonl")
        lines = []

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def wide_legs(dec, prompts, names):
            legs = {"lanes-8": (8, lambda n: dec.generate_batch(prompts[:8], n, lanes=8, lane_context=ctx))}
            for w in (16, 32, 64):
                legs[f"wide-{w}"] = (w, (lambda w: lambda n: dec.generate_wide(prompts[:w], n, lanes=w, lane_context=ctx))(w))
            legs = {k: v for k, v in legs.items() if k in names}
            for _, fn in legs.values():
                fn(12)
            rows = {}
            for rep in range(2):
                for name, (width, fn) in legs.items():
                    dt, outs = window(lambda: fn(n_new), lambda: fn(1))
                    assert all(len(o) == n_new for o in outs)
                    rows.setdefault(name, []).append({"tokens_per_s": round(width * (n_new - 1) / dt, 1), "ms_per_step": round(dt * 1e3 / (n_new - 1), 4)})
            return {k: max(v, key=lambda r: r["tokens_per_s"]) for k, v in rows.items()}

        def prompt_ms(dec, ids):
            ts = []
            for _ in range(6):
                dec.reset()
                t0 = time.perf_counter()
                dec.forward(ids, fetch=False)
                ts.append((time.perf_counter() - t0) * 1e3)
            return round(float(np.median(ts[1:])), 3)

        def shape(label, fdir, bdir, vocab_lo, vocab_hi):
            prompts = [rng.integers(vocab_lo, vocab_hi, 128).tolist() for _ in range(64)]
            long_ids = {n: rng.integers(vocab_lo, vocab_hi, n).tolist() for n in (128, 384)}
            fdec = kjarni_amd.HipDecoder(fdir, max_context=2048)
            off = wide_legs(fdec, prompts, ("lanes-8",))
            p_off = {n: prompt_ms(fdec, ids) for n, ids in long_ids.items()}
            fdec.set_fp8_matrix_cores(True)
            on = wide_legs(fdec, prompts, ("lanes-8", "wide-16", "wide-32", "wide-64"))
            p_on = {n: prompt_ms(fdec, ids) for n, ids in long_ids.items()}
            fbytes = fdec.weight_bytes
            del fdec
            bdec = kjarni_amd.HipDecoder(bdir, max_context=2048)
            bf = wide_legs(bdec, prompts, ("lanes-8", "wide-16", "wide-32", "wide-64"))
            p_bf = {n: prompt_ms(bdec, ids) for n, ids in long_ids.items()}
            bbytes = bdec.weight_bytes
            del bdec
            wides = ("wide-16", "wide-32", "wide-64")
            line = {"metric": f"aggregate tokens/sec greedy decode in wide lanes, {label}, FP8 e4m3 weights on the bf16 matrix cores",
                    "unit": "tokens/s", "value": on["wide-64"]["tokens_per_s"], "n_gpus": 1, "data": "synthetic",
                    "dtype": "F8_E4M3 layer weights + f32 scales, bf16 table / head, f32 activations/accumulate/KV",
                    "config": {"workload": f"{label}, random codes, one 128-token prompt per lane, {n_new} generated tokens per lane, lane_context "
                                           f"{ctx}; every leg twice in one process, best of two"},
                    "fp8_switch_off": off, "fp8_switch_on": on, "bf16_same_shape": bf,
                    "x_fp8_lanes_8": {k: round(on[k]["tokens_per_s"] / off["lanes-8"]["tokens_per_s"], 3) for k in wides},
                    "x_bf16_same_width": {k: round(on[k]["tokens_per_s"] / bf[k]["tokens_per_s"], 3) for k in wides},
                    "prompt_ms": {"fp8_switch_off": p_off, "fp8_switch_on": p_on, "bf16": p_bf},
                    "prompt_x_switch_off": {n: round(p_on[n] / p_off[n], 3) for n in p_on},
                    "prompt_x_bf16": {n: round(p_on[n] / p_bf[n], 3) for n in p_on},
                    "weight_bytes": {"fp8": fbytes, "bf16": bbytes}}
            emit(line)
            lines.append(line)

        fcfg = dict(synth.LLAMA_1B, max_position_embeddings=4096, eos_token_id=synth.LLAMA_1B["vocab_size"] + 1)
        fdir, bdir = os.path.join(tmp, "llama-1b-fp8-wide"), os.path.join(tmp, "llama-1b-bf16-wide")
        fp8_fixture.fp8_model(fdir, fcfg, "channel", seed=0, keep_hf=False)
        synth.llm_model(bdir, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        shape("Llama-3.2-1B shape, per-channel scales", fdir, bdir, 1000, 100000)
        q3 = dict(fp8_fixture.QWEN3_06B, max_position_embeddings=4096, eos_token_id=fp8_fixture.QWEN3_06B["vocab_size"] + 1)
        fdir, bdir = os.path.join(tmp, "qwen3-06b-fp8-wide"), os.path.join(tmp, "qwen3-06b-bf16-wide")
        fp8_fixture.fp8_model(fdir, q3, "block", seed=0, keep_hf=False)
        qwen3_fixture.qwen3_model(bdir, q3, seed=0, store_bf16=True)
        shape("Qwen3-0.6B shape, 128 x 128 block scales", fdir, bdir, 1000, 100000)
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_lookup" in which:
        # Method (measuring guide, section 5; as llm_lanes): one process on one box; the plain step graph, the verify hook at
        # every row count and the lookup graphs are warmed first; then plain generate() -- the yardstick -- alternates with the
        # verify-step loops (2 / 4 / 8 rows) and generate_lookup (draft_tokens 1 / 3 / 7 = 2 / 4 / 8 rows), twice.  A decode window
        # is a whole generation minus the same call cut after its first token (prefill and first pick).
        from tests import gpt2_fixture
        from tests import lookup_cases
        rng = np.random.default_rng(0)
        trace_steps = int(os.environ.get("KJARNI_LOOKUP_STEPS", "0"))
        ROWS = (2, 4, 8)

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def verify_loop(dec, prompt, draft, rows, steps):
            """ms per verify_step call: a fixed draft, so the acceptance (and the time) does not depend on the weights' values."""
            dec.reset()
            dec.forward(prompt, fetch=False)
            t0 = time.perf_counter()
            for _ in range(steps):
                dec.verify_step(prompt[-1], draft[:rows - 1], rows)
            return (time.perf_counter() - t0) * 1e3 / steps

        def measure(label, dec, prompt, n_new, dtype):
            draft = prompt[:7]
            if trace_steps:  # a short run for rocprofv3 --kernel-trace --stats: trace_steps verify steps of 8 rows
                verify_loop(dec, prompt, draft, 8, trace_steps)
                return
            dec.generate(prompt, 8)
            for rows in ROWS:
                verify_loop(dec, prompt, draft, rows, 8)
                dec.generate_lookup(prompt, 40, draft_tokens=rows - 1)
            plain_ms, plain_rate, hook, replay, e2e = [], [], {}, {}, {}
            hist = {}
            for rep in range(2):
                for rows in ROWS:
                    dt, out = window(lambda: dec.generate(prompt, n_new), lambda: dec.generate(prompt, 1))
                    assert len(out) == n_new
                    plain_ms.append(dt * 1e3 / (n_new - 1))
                    plain_rate.append((n_new - 1) / dt)
                    hook.setdefault(rows, []).append(verify_loop(dec, prompt, draft, rows, 64))
                    dt, (got, st) = window(lambda: dec.generate_lookup(prompt, n_new, draft_tokens=rows - 1),
                                           lambda: dec.generate_lookup(prompt, 1, draft_tokens=rows - 1))
                    assert len(got) == n_new
                    same = got == out
                    steps = st["verify_steps"] + st["single_row_steps"]
                    replay.setdefault(rows, []).append(dt * 1e3 / steps)
                    e2e.setdefault(rows, []).append({"tokens_per_s": round((n_new - 1) / dt, 1), "verify_steps": steps,
                                                     "drafted": st["drafted_tokens"], "accepted": st["accepted_tokens"],
                                                     "ids_equal_plain": same})
                    h = {}
                    for _, a in lookup_cases.simulate(prompt, got, (rows - 1, 3, 1)):
                        h[a] = h.get(a, 0) + 1
                    hist[rows] = {str(k): h[k] for k in sorted(h)}
            plain = float(np.median(plain_ms))
            med = lambda xs: float(np.median(xs))  # noqa: E731
            emit({"metric": f"prompt-lookup decoding, {label}", "unit": "ms per step", "value": round(med(replay[8]), 4), "n_gpus": 1,
                  "dtype": dtype, "data": "synthetic",
                  "config": {"workload": f"{label}, random init, one 128-token prompt, {n_new} generated tokens; plain generate() alternated "
                                         "twice with verify-step loops and generate_lookup at 2 / 4 / 8 rows in one process",
                             "note": "random-init greedy output degenerates into repetition: the end-to-end rows are the full-acceptance "
                                     "end of the range, not a workload"},
                  "plain_ms_per_step": {"median": round(plain, 4), "min": round(min(plain_ms), 4), "max": round(max(plain_ms), 4),
                                        "runs": [round(x, 4) for x in plain_ms]},
                  "plain_tokens_per_s": round(med(plain_rate), 1),
                  "verify_ms_per_step_hook": {str(r): [round(x, 4) for x in hook[r]] for r in ROWS},        # uncaptured, host sync per step
                  "verify_ms_per_step_replayed": {str(r): [round(x, 4) for x in replay[r]] for r in ROWS},  # inside generate_lookup
                  "verify_over_plain_replayed": {str(r): round(med(replay[r]) / plain, 3) for r in ROWS},
                  "break_even_accepted_per_step_replayed": {str(r): round(med(replay[r]) / plain - 1, 3) for r in ROWS},
                  "break_even_accepted_per_step_hook": {str(r): round(med(hook[r]) / plain - 1, 3) for r in ROWS},
                  "generate_lookup": {str(r): e2e[r] for r in ROWS}, "accepted_histogram": {str(r): hist[r] for r in ROWS},
                  "x_plain_tokens_per_s": {str(r): round(max(x["tokens_per_s"] for x in e2e[r]) / med(plain_rate), 2) for r in ROWS},
                  "weight_bytes": dec.weight_bytes})

        d = os.path.join(tmp, "llama-1b-lookup")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, rng.integers(1000, 100000, 128).tolist(), 512,
                "bf16 weights, f32 activations/accumulate/KV")
        del dec
        if not trace_steps:  # (the trace run is the Llama shape alone)
            gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
            gd = os.path.join(tmp, "gpt2-small-lookup")
            gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
            dec = kjarni_amd.HipDecoder(gd)
            measure("gpt2-small shape, bf16 weights", dec, rng.integers(0, 50257, 128).tolist(), 512,
                    "bf16 weights, f32 activations/accumulate/KV")
            del dec

    if "llm_lookup_sampled" in which:
        # Method (as llm_lookup): one process on one box, everything warmed first; the plain sampled loop -- the yardstick --
        # alternates with verify-and-cut steps (the hook: verify pass, rows penalty, rows cut, one copy, one synchronise, the host's
        # decision) at 2 / 4 / 8 rows and with the sampled lookup loop, twice, at the family's default sampling config.  Every
        # figure is a median over runs that end in a synchronise.  The two ends of acceptance are steered by the draws: u = 0
        # takes token 0 whatever the distribution (sample_from_probs), so the output repeats and every drafted token is accepted;
        # seeded draws over a random-init model give an output that hardly repeats, so next to nothing is drafted or accepted
        # (not steered to exactly none: that needs every step's distribution; the line reports what was drafted and accepted).
        from tests import gpt2_fixture
        from tests import sampled_lookup_cases as SC
        rng = np.random.default_rng(0)
        ROWS = (2, 4, 8)

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, prompt, n_new, dtype, family):
            p = dict(SC.FAMILY_DEFAULTS[family])
            kw = dict(temperature=p["temperature"], top_k=p["top_k"], top_p=p["top_p"], min_p=p["min_p"],
                      repetition_penalty=p["repetition_penalty"])
            zeros = np.zeros(n_new, np.float32)
            seeded = np.random.default_rng(1).random(n_new).astype(np.float32)
            draft = prompt[:7]

            def hook_loop(rows, steps):
                dec.reset()
                dec.forward(prompt, fetch=False)
                t0 = time.perf_counter()
                for _ in range(steps):
                    dec.verify_step_sampled(prompt[-1], draft[:rows - 1], zeros[:rows], rows=rows, history=prompt, fetch=False, **kw)
                return (time.perf_counter() - t0) * 1e3 / steps

            dec.generate_sampled(prompt, 8, uniforms=seeded[:8], **kw)
            for rows in ROWS:
                hook_loop(rows, 8)
                dec.generate_sampled(prompt, 40, lookup=(rows - 1, 3, 1), uniforms=zeros[:40], **kw)
            plain_ms, plain_rate, hook, e2e = [], [], {}, {}
            for rep in range(2):
                for rows in ROWS:
                    dt, (out, _) = window(lambda: dec.generate_sampled(prompt, n_new, uniforms=seeded, **kw),
                                          lambda: dec.generate_sampled(prompt, 1, uniforms=seeded[:1], **kw))
                    plain_ms.append(dt * 1e3 / max(len(out) - 1, 1))
                    plain_rate.append(max(len(out) - 1, 1) / dt)
                    hook.setdefault(rows, []).append(hook_loop(rows, 64))
                    for end, u in (("all_accepted", zeros), ("none_accepted", seeded)):
                        dt, (got, st) = window(lambda: dec.generate_sampled(prompt, n_new, lookup=(rows - 1, 3, 1), uniforms=u, **kw),
                                               lambda: dec.generate_sampled(prompt, 1, lookup=(rows - 1, 3, 1), uniforms=u[:1], **kw))
                        steps = st["verify_steps"] + st["single_row_steps"]
                        same = got == dec.generate_sampled(prompt, n_new, uniforms=u, **kw)[0]
                        e2e.setdefault(end, {}).setdefault(rows, []).append(
                            {"tokens_per_s": round(max(len(got) - 1, 1) / dt, 1), "ms_per_step": round(dt * 1e3 / max(steps, 1), 4),
                             "steps": steps, "drafted": st["drafted_tokens"], "accepted": st["accepted_tokens"], "tokens": len(got),
                             "ids_equal_plain": same})
            med = lambda xs: float(np.median(xs))  # noqa: E731
            plain = med(plain_ms)
            c, l = dec.sampling_routes()
            emit({"metric": f"sampled prompt-lookup decoding, {label}", "unit": "ms per step",
                  "value": round(med([x["ms_per_step"] for x in e2e["all_accepted"][8]]), 4), "n_gpus": 1,
                  "dtype": dtype, "data": "synthetic",
                  "config": {"workload": f"{label}, random init, one 128-token prompt, {n_new} generated tokens, {family} default sampling "
                                         f"{kw}; the plain sampled loop alternated twice with verify-and-cut steps and the sampled "
                                         "lookup loop at 2 / 4 / 8 rows in one process"},
                  "plain_sampled_ms_per_step": {"median": round(plain, 4), "min": round(min(plain_ms), 4), "max": round(max(plain_ms), 4),
                                                "runs": [round(x, 4) for x in plain_ms]},
                  "plain_sampled_tokens_per_s": round(med(plain_rate), 1),
                  # the loop's own step (captured chain, one copy, one synchronise, the host's decision): whole windows of the
                  # all-accepted runs over their steps; the hook is uncaptured and re-uploads ids and position every call
                  "verify_and_cut_ms_per_step_replayed": {str(r): [x["ms_per_step"] for x in e2e["all_accepted"][r]] for r in ROWS},
                  "verify_and_cut_over_plain_replayed": {str(r): round(med([x["ms_per_step"] for x in e2e["all_accepted"][r]]) / plain, 3)
                                                         for r in ROWS},
                  "break_even_accepted_per_step_replayed": {str(r): round(med([x["ms_per_step"] for x in e2e["all_accepted"][r]]) / plain - 1, 3)
                                                            for r in ROWS},
                  "verify_and_cut_ms_per_step_hook": {str(r): [round(x, 4) for x in hook[r]] for r in ROWS},
                  "break_even_accepted_per_step_hook": {str(r): round(med(hook[r]) / plain - 1, 3) for r in ROWS},
                  "generate_lookup_sampled": {end: {str(r): e2e[end][r] for r in ROWS} for end in e2e},
                  "x_plain_tokens_per_s": {end: {str(r): round(max(x["tokens_per_s"] for x in e2e[end][r]) / med(plain_rate), 2) for r in ROWS}
                                           for end in e2e},
                  "rows_from_candidates": c, "rows_from_logits": l, "weight_bytes": dec.weight_bytes})

        d = os.path.join(tmp, "llama-1b-lookup-sampled")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, rng.integers(1000, 100000, 128).tolist(), 512,
                "bf16 weights, f32 activations/accumulate/KV", "llama")
        del dec
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small-lookup-sampled")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        dec = kjarni_amd.HipDecoder(gd)
        measure("gpt2-small shape, bf16 weights", dec, rng.integers(1, 50257, 128).tolist(), 512,
                "bf16 weights, f32 activations/accumulate/KV", "gpt2")
        del dec

    if "llm_draft" in which:
        # Method (as llm_lookup): one process on one box; the Llama-3.2-1B shape (bf16, random init) as target, everything warmed
        # first; plain generate() of the target -- the yardstick -- alternates with generate_lookup (the verify step of the same
        # row count, replayed), the drafter's own plain generate() (its step) and generate_draft at 2 / 4 / 8 rows, twice.  A decode
        # window is a whole generation minus the same call cut after its first token.  The round time does not depend on what is
        # accepted; the end-to-end rows are the two ends random weights allow -- a copy of the target as drafter (every draft
        # accepted: the ceiling) and an unrelated checkpoint (next to nothing accepted: the floor; what it accepts is in the
        # line) -- ends of a range, not workloads.  A drafter of the same width with 4 layers gives the per-round cost of a
        # cheaper drafter only.
        rng = np.random.default_rng(0)
        ROWS = (2, 4, 8)
        n_new = int(os.environ.get("KJARNI_DRAFT_TOKENS", "256"))

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        med = lambda xs: float(np.median(xs))  # noqa: E731
        prompt = rng.integers(1000, 100000, 128).tolist()
        d = os.path.join(tmp, "llama-1b-draft-target")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        d_other = os.path.join(tmp, "llama-1b-draft-other")
        synth.llm_model(d_other, synth.LLAMA_1B, seed=1, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        d_shallow = os.path.join(tmp, "llama-1b-draft-shallow")
        synth.llm_model(d_shallow, synth.LLAMA_1B, seed=2, store_bf16=True, max_position_embeddings=4096, eos_token_id=[], num_hidden_layers=4)
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        drafters = {"copy of the target": kjarni_amd.HipDecoder(d, max_context=2048),
                    "unrelated checkpoint, same shape": kjarni_amd.HipDecoder(d_other, max_context=2048),
                    "same width, 4 layers": kjarni_amd.HipDecoder(d_shallow, max_context=2048)}
        dec.generate(prompt, 8)
        for rows in ROWS:
            dec.generate_lookup(prompt, 40, draft_tokens=rows - 1)
        for drf in drafters.values():
            drf.generate(prompt, 8)
            for rows in ROWS:
                dec.generate_draft(drf, prompt, 40, rows - 1)
        plain_ms, plain_rate, verify_ms = [], [], {r: [] for r in ROWS}
        step_ms = {k: [] for k in drafters}
        round_ms = {k: {r: [] for r in ROWS} for k in drafters}
        e2e = {k: {r: [] for r in ROWS} for k in drafters}
        for rep in range(2):
            dt, out = window(lambda: dec.generate(prompt, n_new), lambda: dec.generate(prompt, 1))
            assert len(out) == n_new
            plain_ms.append(dt * 1e3 / (n_new - 1))
            plain_rate.append((n_new - 1) / dt)
            for rows in ROWS:
                dt, (got, st) = window(lambda: dec.generate_lookup(prompt, n_new, draft_tokens=rows - 1),
                                       lambda: dec.generate_lookup(prompt, 1, draft_tokens=rows - 1))
                verify_ms[rows].append(dt * 1e3 / (st["verify_steps"] + st["single_row_steps"]))
            for name, drf in drafters.items():
                dt, dout = window(lambda: drf.generate(prompt, n_new), lambda: drf.generate(prompt, 1))
                step_ms[name].append(dt * 1e3 / (n_new - 1))
                for rows in ROWS:
                    dt, (got, st) = window(lambda: dec.generate_draft(drf, prompt, n_new, rows - 1),
                                           lambda: dec.generate_draft(drf, prompt, 1, rows - 1))
                    assert len(got) == n_new
                    rounds = st["verify_steps"] + st["single_row_steps"]
                    round_ms[name][rows].append(dt * 1e3 / rounds)
                    e2e[name][rows].append({"tokens_per_s": round((n_new - 1) / dt, 1), "rounds": rounds, "drafted": st["drafted_tokens"],
                                            "accepted": st["accepted_tokens"], "ids_equal_plain": got == out})
        plain = med(plain_ms)
        for name in drafters:
            parts = {r: med(verify_ms[r]) + (r - 1) * med(step_ms[name]) for r in ROWS}   # (b): what the chain is made of
            emit({"metric": f"draft-model decoding, Llama-3.2-1B shape target, drafter: {name}", "unit": "ms per round",
                  "value": round(med(round_ms[name][8]), 4), "n_gpus": 1, "dtype": "bf16 weights, f32 activations/accumulate/KV",
                  "data": "synthetic",
                  "config": {"workload": f"random init, one 128-token prompt, {n_new} generated tokens; plain generate(), generate_lookup, the "
                                         "drafter's generate() and generate_draft at 2 / 4 / 8 rows alternated twice in one process",
                             "note": "the end-to-end rows are ends of a range (what a random-init drafter happens to accept), not workloads; "
                                     "the round time does not depend on the acceptance"},
                  "plain_ms_per_step": {"median": round(plain, 4), "runs": [round(x, 4) for x in plain_ms]},
                  "plain_tokens_per_s": round(med(plain_rate), 1),
                  "drafter_ms_per_step": {"median": round(med(step_ms[name]), 4), "runs": [round(x, 4) for x in step_ms[name]]},
                  "verify_ms_per_step_replayed": {str(r): [round(x, 4) for x in verify_ms[r]] for r in ROWS},
                  "round_ms_replayed": {str(r): [round(x, 4) for x in round_ms[name][r]] for r in ROWS},
                  "round_over_plain": {str(r): round(med(round_ms[name][r]) / plain, 3) for r in ROWS},
                  "verify_plus_drafter_steps_ms": {str(r): round(parts[r], 4) for r in ROWS},
                  "round_over_verify_plus_drafter_steps": {str(r): round(med(round_ms[name][r]) / parts[r], 3) for r in ROWS},
                  "break_even_accepted_per_round": {str(r): round(med(round_ms[name][r]) / plain - 1, 3) for r in ROWS},
                  "generate_draft": {str(r): e2e[name][r] for r in ROWS},
                  "x_plain_tokens_per_s": {str(r): round(max(x["tokens_per_s"] for x in e2e[name][r]) / med(plain_rate), 2) for r in ROWS},
                  "weight_bytes": dec.weight_bytes, "drafter_weight_bytes": drafters[name].weight_bytes})
        del dec, drafters

    if "llm_score" in which:
        # Method (measuring guide, section 5; as llm_lookup): one process on one box; forward() -- the yardstick --, score() on
        # the fused route and score() on the rows route are warmed first, then alternated twice; every run ends in a
        # synchronise (forward() and score() return after one), medians over the runs.  KJARNI_SCORE_TRACE=N: N fused score()
        # calls of the 2 048-token prompt on the Llama shape only (for a kernel trace of its own).
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        trace_calls = int(os.environ.get("KJARNI_SCORE_TRACE", "0"))
        LENS = (128, 2048)

        def run_ms(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def measure(label, dec, vocab, lo, dtype):
            prompts = {n: rng.integers(lo, vocab, n).tolist() for n in LENS}
            if trace_calls:
                for _ in range(trace_calls):
                    dec.score(prompts[2048])
                return

            def fwd(ids):
                dec.reset()
                dec.forward(ids, fetch=False)

            def score(ids, fused):
                dec.set_score_fused(fused)
                dec.score(ids)
            for n in LENS:
                fwd(prompts[n])
                score(prompts[n], True)
                score(prompts[n], False)
            runs = {(kind, n): [] for kind in ("forward", "fused", "rows") for n in LENS}
            for rep in range(2):
                for n in LENS:
                    for _ in range(3):
                        runs[("forward", n)].append(run_ms(lambda: fwd(prompts[n])))
                        runs[("fused", n)].append(run_ms(lambda: score(prompts[n], True)))
                        runs[("rows", n)].append(run_ms(lambda: score(prompts[n], False)))
            dec.set_score_fused(True)
            med = lambda xs: float(np.median(xs))  # noqa: E731
            out = {}
            for n in LENS:
                f, a, b = med(runs[("forward", n)]), med(runs[("fused", n)]), med(runs[("rows", n)])
                out[str(n)] = {"forward_ms": round(f, 3), "score_fused_ms": round(a, 3), "score_rows_ms": round(b, 3),
                               "head_added_fused_ms": round(a - f, 3), "head_added_rows_ms": round(b - f, 3),
                               "rows_over_fused_added": round((b - f) / (a - f), 2) if a > f else None,
                               "head_gflop": round(2.0 * (n - 1) * vocab * dec.hidden / 1e9, 2),
                               "runs": {k: [round(x, 3) for x in runs[(k, n)]] for k in ("forward", "fused", "rows")}}
            emit({"metric": f"scoring, {label}", "unit": "ms added by the head at 2048 tokens (fused)", "value": out["2048"]["head_added_fused_ms"],
                  "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                  "config": {"workload": f"{label}, random init; forward() of a 128- and a 2 048-token prompt against score() of the same ids "
                                         "(first = 1) on the fused and on the rows route, alternated twice in one process, medians of 6 runs, "
                                         "every run ends in a synchronise"},
                  "lengths": out, "weight_bytes": dec.weight_bytes})

        d = os.path.join(tmp, "llama-1b-score")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, 100000, 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        if not trace_calls:  # (the trace run is the Llama shape alone)
            gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=2048, vocab_size=50257, eos_token_id=None)
            gd = os.path.join(tmp, "gpt2-small-score")
            gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
            dec = kjarni_amd.HipDecoder(gd)
            measure("gpt2-small shape, bf16 weights (n_ctx 2048)", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
            del dec

    if "llm_score_topk" in which:
        # Method (measuring guide, section 5; as llm_score): one process on one box; score() -- the yardstick, the code before
        # score_topk() existed -- and score_topk() at top_k = 1 and 8 are warmed first, then alternated twice, three runs each;
        # every run ends in a synchronise (both return after one), medians over the 6 runs of a kind.
        rng = np.random.default_rng(0)
        d = os.path.join(tmp, "llama-1b-score-topk")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        kinds = {"score": lambda ids: dec.score(ids), "topk1": lambda ids: dec.score_topk(ids, 1, 1), "topk8": lambda ids: dec.score_topk(ids, 1, 8)}
        lines = []
        for n in (128, 2048):
            ids = rng.integers(1000, 100000, n).tolist()
            for fused in (True, False):
                dec.set_score_fused(fused)
                for fn in kinds.values():
                    fn(ids)
                runs = {k: [] for k in kinds}
                for rep in range(2):
                    for _ in range(3):
                        for k, fn in kinds.items():
                            t0 = time.perf_counter()
                            fn(ids)
                            runs[k].append((time.perf_counter() - t0) * 1e3)
                med = {k: float(np.median(v)) for k, v in runs.items()}
                line = {"metric": f"score_topk / score, Llama-3.2-1B shape, bf16 weights, {n} tokens, {'fused' if fused else 'rows'} route",
                        "value": round(med["topk8"] / med["score"], 4), "unit": "ratio of medians at top_k = 8", "n_gpus": 1,
                        "dtype": "bf16 weights, f32 activations/accumulate/KV", "data": "synthetic",
                        "config": {"workload": f"random init; score() against score_topk() at top_k 1 and 8 of the same {n} ids (first = 1), "
                                               "alternated twice in one process, medians of 6 runs, every run ends in a synchronise"},
                        "tokens": n, "route": "fused" if fused else "rows", "score_ms": round(med["score"], 3),
                        "score_topk1_ms": round(med["topk1"], 3), "score_topk8_ms": round(med["topk8"], 3),
                        "topk1_over_score": round(med["topk1"] / med["score"], 4), "topk8_over_score": round(med["topk8"] / med["score"], 4),
                        "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
                emit(line)
                lines.append(line)
        dec.set_score_fused(True)
        del dec
        with open(os.path.join(ROOT, "profiles", "llm_score_topk_bench.jsonl"), "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_score_batch" in which:
        # Method (measuring guide, section 5; as llm_score): one process on one box; every leg of a case is warmed first, then the
        # legs are alternated twice, two runs each; every run ends in a synchronise (score_batch() and score() return after one);
        # medians over the 4 runs of a leg.  The score() loop over the same sequences is what there was before score_batch().
        rng = np.random.default_rng(0)
        d = os.path.join(tmp, "llama-1b-score-batch")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        dtype = "bf16 weights, f32 activations/accumulate"
        method = "random init; legs alternated twice in one process, medians of 4 runs, every run ends in a synchronise"
        lines = []

        def flat_of(seqs):
            return (np.concatenate(seqs).astype(np.uint32), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32))

        def measure(legs):
            for fn in legs.values():
                fn()
            runs = {k: [] for k in legs}
            for rep in range(2):
                for _ in range(2):
                    for k, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        runs[k].append((time.perf_counter() - t0) * 1e3)
            return {k: float(np.median(v)) for k, v in runs.items()}, runs

        def loop_of(seqs, firsts):
            def loop():
                for s, f in zip(seqs, firsts):
                    dec.score(s, f)
            return loop

        for n in (8, 64, 256):      # (a) N x 128 tokens, every token scored
            seqs = [rng.integers(1000, 100000, 128).astype(np.uint32) for _ in range(n)]
            firsts = np.ones(n, np.int32)
            flat, off = flat_of(seqs)
            med, runs = measure({"score_batch": lambda: dec.score_batch_flat(flat, off, firsts), "score_loop": loop_of(seqs, firsts)})
            line = {"metric": f"score loop / score_batch, Llama-3.2-1B shape, bf16 weights, {n} x 128 tokens, first = 1",
                    "value": round(med["score_loop"] / med["score_batch"], 2), "unit": "ratio of medians", "n_gpus": 1, "dtype": dtype,
                    "data": "synthetic", "config": {"workload": method}, "sequences": n, "score_batch_ms": round(med["score_batch"], 3),
                    "score_loop_ms": round(med["score_loop"], 3), "tokens_per_s_score_batch": round(n * 128 / med["score_batch"] * 1e3, 1),
                    "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
            emit(line)
            lines.append(line)

        def choice_case(n_ctx, ctx_len, n_cont, cont_len):
            """(shared, distinct): n_ctx contexts x n_cont continuations; distinct = the same batch with every sequence's token 0 made
            its own, so that neighbours share nothing at the same shapes."""
            shared, distinct = [], []
            for c in range(n_ctx):
                ctx = rng.integers(1000, 100000, ctx_len).astype(np.uint32)
                for k in range(n_cont):
                    s = np.concatenate([ctx, rng.integers(1000, 100000, cont_len).astype(np.uint32)])
                    shared.append(s)
                    t = s.copy()
                    t[0] = 100 + len(distinct)
                    distinct.append(t)
            return shared, distinct, np.full(n_ctx * n_cont, ctx_len, np.int32)

        # (b) multiple choice, 64 contexts of 256 tokens x 4 continuations of 16; and shorter contexts, for kScoreMinShared
        for ctx_len in (256, 64, 16, 4, 1):
            shared, distinct, firsts = choice_case(64, ctx_len, 4, 16)
            (fs, os_), (fd, od) = flat_of(shared), flat_of(distinct)
            legs = {"shared": lambda: dec.score_batch_flat(fs, os_, firsts), "not_shared": lambda: dec.score_batch_flat(fd, od, firsts)}
            if ctx_len == 256:
                legs["score_loop"] = loop_of(shared, firsts)
            r0 = dec.score_batch_rows()
            dec.score_batch_flat(fs, os_, firsts)
            r1 = dec.score_batch_rows()
            dec.score_batch_flat(fd, od, firsts)
            r2 = dec.score_batch_rows()
            med, runs = measure(legs)
            line = {"metric": f"not sharing / sharing, Llama-3.2-1B shape, bf16 weights, 64 contexts of {ctx_len} x 4 continuations of 16 tokens",
                    "value": round(med["not_shared"] / med["shared"], 3), "unit": "ratio of medians", "n_gpus": 1, "dtype": dtype,
                    "data": "synthetic", "config": {"workload": method + "; not_shared: every sequence's token 0 made distinct"},
                    "context_tokens": ctx_len, "shared_ms": round(med["shared"], 3), "not_shared_ms": round(med["not_shared"], 3),
                    "rows_shared": r1[0] - r0[0], "rows_saved_shared": r1[1] - r0[1], "rows_not_shared": r2[0] - r1[0],
                    "rows_saved_not_shared": r2[1] - r1[1], "min_shared": kjarni_amd.decoder.SCORE_MIN_SHARED,
                    "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
            if "score_loop" in med:
                line["score_loop_ms"] = round(med["score_loop"], 3)
                line["score_loop_over_shared"] = round(med["score_loop"] / med["shared"], 2)
            emit(line)
            lines.append(line)
        # (c) the same multiple choice behind a BOS token every sequence starts with (what a tokenizer that prepends BOS gives):
        # as planned, against the same batch with the first token made distinct per context, so that no two contexts share it
        for ctx_len in (64, 16):
            shared, _, firsts = choice_case(64, ctx_len, 4, 16)
            bos = [s.copy() for s in shared]
            for s in bos:
                s[0] = 1
            (fb, ob), (fs, os_) = flat_of(bos), flat_of(shared)
            r0 = dec.score_batch_rows()
            dec.score_batch_flat(fb, ob, firsts)
            r1 = dec.score_batch_rows()
            dec.score_batch_flat(fs, os_, firsts)
            r2 = dec.score_batch_rows()
            med, runs = measure({"common_first_token": lambda: dec.score_batch_flat(fb, ob, firsts),
                                 "first_token_per_context": lambda: dec.score_batch_flat(fs, os_, firsts)})
            line = {"metric": f"common first token / first token per context, Llama-3.2-1B shape, bf16 weights, 64 contexts of {ctx_len} x 4 "
                              "continuations of 16 tokens", "value": round(med["common_first_token"] / med["first_token_per_context"], 3),
                    "unit": "ratio of medians", "n_gpus": 1, "dtype": dtype, "data": "synthetic", "config": {"workload": method},
                    "context_tokens": ctx_len, "common_first_token_ms": round(med["common_first_token"], 3),
                    "first_token_per_context_ms": round(med["first_token_per_context"], 3), "rows_common_first_token": r1[0] - r0[0],
                    "rows_saved_common_first_token": r1[1] - r0[1], "rows_first_token_per_context": r2[0] - r1[0],
                    "rows_saved_first_token_per_context": r2[1] - r1[1], "min_shared": kjarni_amd.decoder.SCORE_MIN_SHARED,
                    "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
            emit(line)
            lines.append(line)
        del dec
        with open(os.path.join(ROOT, "profiles", "llm_score_batch_bench.jsonl"), "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_prefix" in which:
        # Method (measuring guide, section 5; as llm_score): one process on one box; every case is warmed with reuse off and on,
        # then off and on are alternated twice, three runs each; a run is set up untimed (the cache brought to the state the case
        # starts from) and ends in a synchronise (generate(), score() and generate_batch() return after one); medians.
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        out_path = os.path.join(ROOT, "profiles", "llm_prefix_bench.jsonl")
        lines = []

        def run_ms(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        def measure(label, dec, vocab, lo, dtype):
            ids = lambda n: rng.integers(lo, vocab, n).tolist()  # noqa: E731
            cases = {}
            for h in (512, 2048):   # turn 2: the history is resident, the message is new
                hist, msg = ids(h), ids(32)
                cases[f"turn2_ttft_history_{h}"] = (lambda hist=hist: dec.generate(hist, 0), lambda hist=hist, msg=msg: dec.generate(hist + msg, 1))
            ctx, conts = ids(512), [ids(8) for _ in range(5)]

            def five_scores():
                for c in conts:
                    dec.score(ctx + c, first=len(ctx))
            cases["five_scores_context_512"] = (dec.reset, five_scores)
            shared = ids(512)
            prompts = [shared + ids(16) for _ in range(8)]
            batch = lambda: dec.generate_batch(prompts, 16, lanes=8, lane_context=1024)  # noqa: E731
            cases["lanes_8_shared_512_cold"] = (dec.reset, batch)
            cases["lanes_8_shared_512_prefix_resident"] = (lambda: dec.generate(shared, 0), batch)
            runs = {(name, on): [] for name in cases for on in (False, True)}
            for on in (False, True):   # warm: allocations, graphs
                dec.set_prefix_reuse(on)
                for setup, fn in cases.values():
                    setup()
                    fn()
            for rep in range(2):
                for on in (False, True):
                    dec.set_prefix_reuse(on)
                    for name, (setup, fn) in cases.items():
                        for _ in range(3):
                            setup()
                            runs[(name, on)].append(run_ms(fn))
            dec.set_prefix_reuse(False)
            med = lambda xs: float(np.median(xs))  # noqa: E731
            res = {}
            for name in cases:
                off, on = med(runs[(name, False)]), med(runs[(name, True)])
                res[name] = {"off_ms": round(off, 3), "on_ms": round(on, 3), "off_over_on": round(off / on, 2) if on > 0 else None,
                             "runs_off": [round(x, 3) for x in runs[(name, False)]], "runs_on": [round(x, 3) for x in runs[(name, True)]]}
            line = {"metric": f"prefix reuse, {label}", "unit": "ms to the first token of turn 2, 2 048-token history (reuse on)",
                    "value": res["turn2_ttft_history_2048"]["on_ms"], "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"{label}, random init; prefix reuse off against on, alternated twice in one process, medians of 6 "
                                           "runs, every run set up untimed and ended by a synchronise"},
                    "cases": res, "weight_bytes": dec.weight_bytes}
            lines.append(line)
            emit(line)

        d = os.path.join(tmp, "llama-1b-prefix")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=4096)
        measure("Llama-3.2-1B shape, bf16 weights", dec, 100000, 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=4096, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small-prefix")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        dec = kjarni_amd.HipDecoder(gd)
        measure("gpt2-small shape, bf16 weights (n_ctx 4096)", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_moe" in which:
        # Method: one process on one box.  A random-weight qwen3_moe model at the Qwen3-30B-A3B widths (hidden 2048, 32 / 4 heads of
        # 128, 128 experts of 768, 8 per token, bf16) cut to 4 layers so that the fixture stays near 5 GB, and a dense Qwen3 model of
        # the same widths with intermediate_size = 8 x 768 = 6144: the same active bytes and FLOPs in the FFN, on the existing dense
        # path -- the yardstick.  Both warmed first, then alternated twice: greedy ms / token (a 128-token generation minus the same
        # call cut after its first token) and the 128-token prompt time (forward(), which returns after a synchronise); medians.
        # The ratio is what routing and gathering cost; the sparse step's streamed bytes against the HBM peak says how far it is
        # from streaming its weights.  (Random routers spread tokens evenly over the experts; a trained router is more skewed.)
        import torch as _t
        from safetensors.torch import save_file as _save
        rng = np.random.default_rng(0)
        H, NH, NKV, D, E_, K_, IM, LAYERS, VOC = 2048, 32, 4, 128, 128, 8, 768, 4, 32000
        n_new = int(os.environ.get("KJARNI_MOE_TOKENS", "128"))

        def rand_bf16(*shape):   # bf16 bit patterns, magnitudes 2^-7 .. 2^-4, made as bits: no 10 GB of f32 on the host
            n = int(np.prod(shape))
            bits = (rng.integers(0, 2, n, dtype=np.uint16) << 15) | ((rng.integers(120, 123, n, dtype=np.uint16)) << 7) | rng.integers(0, 128, n, dtype=np.uint16)
            return _t.from_numpy(bits.view(np.int16).reshape(shape)).view(_t.bfloat16)

        def write(path, moe):
            os.makedirs(path, exist_ok=True)
            cfg = dict(model_type="qwen3_moe" if moe else "qwen3", hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=NH,
                       num_key_value_heads=NKV, head_dim=D, intermediate_size=K_ * IM, vocab_size=VOC, max_position_embeddings=4096,
                       rms_norm_eps=1e-6, rope_theta=1000000.0, tie_word_embeddings=True, eos_token_id=[])
            if moe:
                cfg.update(num_experts=E_, num_experts_per_tok=K_, moe_intermediate_size=IM, norm_topk_prob=True, decoder_sparse_step=1,
                           mlp_only_layers=[])
            json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
            ones = lambda n: _t.ones(n, dtype=_t.float32)  # noqa: E731
            t = {"model.embed_tokens.weight": rand_bf16(VOC, H), "model.norm.weight": ones(H)}
            for i in range(LAYERS):
                q = f"model.layers.{i}."
                t[q + "self_attn.q_proj.weight"], t[q + "self_attn.o_proj.weight"] = rand_bf16(NH * D, H), rand_bf16(H, NH * D)
                t[q + "self_attn.k_proj.weight"], t[q + "self_attn.v_proj.weight"] = rand_bf16(NKV * D, H), rand_bf16(NKV * D, H)
                t[q + "self_attn.q_norm.weight"], t[q + "self_attn.k_norm.weight"] = ones(D), ones(D)
                t[q + "input_layernorm.weight"], t[q + "post_attention_layernorm.weight"] = ones(H), ones(H)
                if moe:
                    t[q + "mlp.gate.weight"] = rand_bf16(E_, H)
                    for e in range(E_):
                        for nm, shape in (("gate_proj", (IM, H)), ("up_proj", (IM, H)), ("down_proj", (H, IM))):
                            t[f"{q}mlp.experts.{e}.{nm}.weight"] = rand_bf16(*shape)
                else:
                    for nm, shape in (("gate_proj", (K_ * IM, H)), ("up_proj", (K_ * IM, H)), ("down_proj", (H, K_ * IM))):
                        t[f"{q}mlp.{nm}.weight"] = rand_bf16(*shape)
            _save(t, os.path.join(path, "model.safetensors"))
            return path

        t0 = time.perf_counter()
        decs = {"moe": kjarni_amd.HipDecoder(write(os.path.join(tmp, "moe-30b-a3b-4l"), True), max_context=1024),
                "dense": kjarni_amd.HipDecoder(write(os.path.join(tmp, "dense-6144-4l"), False), max_context=1024)}
        setup_s = time.perf_counter() - t0
        prompt = rng.integers(1000, VOC, 128).tolist()
        step_ms, prompt_ms = {"moe": [], "dense": []}, {"moe": [], "dense": []}

        def once(dec):
            dec.reset()
            t0 = time.perf_counter()
            dec.generate(prompt, 1)
            t1 = time.perf_counter()
            dec.reset()
            out = dec.generate(prompt, n_new)
            t2 = time.perf_counter()
            dec.reset()
            t3 = time.perf_counter()
            dec.forward(prompt, fetch=False)
            t4 = time.perf_counter()
            return ((t2 - t1) - (t1 - t0)) * 1e3 / max(len(out) - 1, 1), (t4 - t3) * 1e3

        for name in ("moe", "dense"):
            once(decs[name])       # warm: captures the step, allocates the prompt workspace
        for _ in range(2):
            for name in ("moe", "dense"):
                for _ in range(3):
                    a, b = once(decs[name])
                    step_ms[name].append(a)
                    prompt_ms[name].append(b)
        med = lambda xs: float(np.median(xs))  # noqa: E731
        attn = ((NH + 2 * NKV) * D * H + H * NH * D) * 2
        moe_tok = LAYERS * (attn + E_ * H * 2 + K_ * 3 * IM * H * 2) + VOC * H * 2          # bytes one sparse step streams
        dense_tok = LAYERS * (attn + 3 * K_ * IM * H * 2) + VOC * H * 2
        emit({"metric": "greedy ms/token and 128-token prompt ms, qwen3_moe at the Qwen3-30B-A3B widths (4 layers, bf16) against a dense "
                        "Qwen3 of the same active FFN bytes", "section": "llm_moe",
              "config": {"hidden": H, "heads": NH, "kv_heads": NKV, "head_dim": D, "experts": E_, "experts_per_tok": K_, "moe_intermediate": IM,
                         "layers": LAYERS, "vocab": VOC, "dense_intermediate": K_ * IM, "tokens": n_new, "prompt": 128},
              "moe_ms_per_token": round(med(step_ms["moe"]), 4), "dense_ms_per_token": round(med(step_ms["dense"]), 4),
              "moe_over_dense_step": round(med(step_ms["moe"]) / med(step_ms["dense"]), 3),
              "moe_prompt_ms": round(med(prompt_ms["moe"]), 3), "dense_prompt_ms": round(med(prompt_ms["dense"]), 3),
              "moe_over_dense_prompt": round(med(prompt_ms["moe"]) / med(prompt_ms["dense"]), 3),
              "moe_streamed_bytes_per_token": moe_tok, "dense_streamed_bytes_per_token": dense_tok,
              "moe_frac_hbm_peak": round(moe_tok / (med(step_ms["moe"]) * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
              "dense_frac_hbm_peak": round(dense_tok / (med(step_ms["dense"]) * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
              "all_step_ms": {k: [round(x, 4) for x in v] for k, v in step_ms.items()},
              "all_prompt_ms": {k: [round(x, 3) for x in v] for k, v in prompt_ms.items()},
              "weight_bytes": {k: d.weight_bytes for k, d in decs.items()}, "fixture_and_load_s": round(setup_s, 1),
              "note": "4 layers: the per-token streams (a few hundred MB) fit the 256 MiB Infinity Cache only in part; the fractions "
                      "may overstate what HBM delivered"})
        del decs

    if "llm_constraint" in which:
        # Method (as llm_lookup): one process on one box, everything warmed first; the plain loop of the same build -- the yardstick
        # -- alternates with the constrained loop, twice, greedy and sampled (the family-neutral config below, one seed).  A decode
        # window is a whole generation minus the same call cut after its first token.  The pattern is [ -~]* over a table in which
        # every token is printable ASCII: nothing is masked, so both loops emit the same ids (asserted) and the difference is the
        # two launches per step (apply, advance) alone.  The mask build: a 100-state pattern, [a-z]{99}, over seeded lower-case
        # tokens of 1..8 bytes at the shape's vocabulary: the whole constructor (upload, kernel, counts, the reachable states) and
        # the kernel entry alone (kjarni_hip_op_constraint_mask: upload, kernel, the mask copied back), medians of 3.
        from kjarni_amd import constraints as KC
        from kjarni_amd import ops as KO
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        n_new = int(os.environ.get("KJARNI_CONSTRAINT_TOKENS", "256"))
        out_path = os.path.join(ROOT, "profiles", "llm_constraint_bench.jsonl")
        lines = []
        med = lambda xs: float(np.median(xs))  # noqa: E731
        SAMPLING = dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.05)

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, vocab, lo, dtype):
            prompt = rng.integers(lo, vocab, 128).tolist()
            con = KC.Constraint(r"[ -~]*", [("t%d " % i).encode() for i in range(vocab)])
            legs = {
                "greedy_plain": lambda n: dec.generate(prompt, n),
                "greedy_constrained": lambda n: dec.generate_constrained(con, prompt, n)[0],
                "sampled_plain": lambda n: dec.generate_sampled(prompt, n, sample=True, seed=7, **SAMPLING)[0],
                "sampled_constrained": lambda n: dec.generate_constrained(con, prompt, n, sample=True, seed=7, **SAMPLING)[0],
            }
            for fn in legs.values():
                fn(8)
            rate = {k: [] for k in legs}
            outs = {}
            for rep in range(2):
                for k, fn in legs.items():
                    dt, out = window(lambda: fn(n_new), lambda: fn(1))
                    assert len(out) == n_new, (k, len(out))
                    rate[k].append((n_new - 1) / dt)
                    outs[k] = out
            assert outs["greedy_plain"] == outs["greedy_constrained"] and outs["sampled_plain"] == outs["sampled_constrained"]
            words = [bytes(rng.integers(97, 123, int(rng.integers(1, 9))).astype(np.uint8)) for _ in range(vocab)]
            rx = KC.Regex(r"[a-z]{99}")
            assert rx.states == 100
            off, data = KC.token_table(words)
            new_ms, op_ms = [], []
            for _ in range(4):   # (the first run of each is the warm-up)
                t0 = time.perf_counter()
                c = KC.Constraint(rx, words)
                new_ms.append((time.perf_counter() - t0) * 1e3)
                c.close()
                t0 = time.perf_counter()
                KO.constraint_mask(rx.trans, off, data)
                op_ms.append((time.perf_counter() - t0) * 1e3)
            g, s = med(rate["greedy_constrained"]) / med(rate["greedy_plain"]), med(rate["sampled_constrained"]) / med(rate["sampled_plain"])
            line = {"metric": f"constrained decoding, {label}", "unit": "constrained / plain tokens per second, greedy", "value": round(g, 4),
                    "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"random init, one 128-token prompt, {n_new} generated tokens; the plain and the constrained loop "
                                           "alternated twice in one process, greedy and sampled (temperature 0.8, top-k 40, top-p 0.9, min-p "
                                           "0.05, one seed); pattern [ -~]* over an all-ASCII table: nothing masked, ids equal (asserted)"},
                    "tokens_per_s": {k: {"median": round(med(v), 1), "runs": [round(x, 1) for x in v]} for k, v in rate.items()},
                    "sampled_constrained_over_plain": round(s, 4),
                    "mask_build_100_states": {"vocab": vocab, "constructor_ms": round(med(new_ms[1:]), 3), "kernel_entry_ms": round(med(op_ms[1:]), 3),
                                              "mask_bytes": 100 * ((vocab + 63) // 64) * 8},
                    "weight_bytes": dec.weight_bytes}
            lines.append(line)
            emit(line)

        d = os.path.join(tmp, "llama-1b-constraint")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, synth.LLAMA_1B["vocab_size"], 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small-constraint")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        dec = kjarni_amd.HipDecoder(gd)
        measure("gpt2-small shape, bf16 weights", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_grammar" in which:
        # Method (as llm_constraint): one process on one box, everything warmed first; three loops alternate twice in one run, greedy
        # and sampled: the plain loop, the pattern route with a pattern that masks nothing ([ -~]* over an all-ASCII table: the
        # parent's route, the yardstick) and the grammar route with the one-rule grammar of the same language.  The grammar route's
        # ids are asserted equal to the plain loop's.  A decode window is a whole generation minus the same call cut after its first
        # token.  The spread is what the two alternations of one loop differ by.  The per-step cost of the two grammar launches is
        # the difference of the grammar and the plain loop's time per token.  For information: json_value on random weights (the
        # run may end early: the tokens it emitted are reported) and the whole GrammarConstraint constructor at V = 128 256.
        from kjarni_amd import constraints as KC
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        n_new = int(os.environ.get("KJARNI_GRAMMAR_TOKENS", "256"))
        out_path = os.path.join(ROOT, "profiles", "llm_grammar_bench.jsonl")
        lines = []
        med = lambda xs: float(np.median(xs))  # noqa: E731
        SAMPLING = dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.05)

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, vocab, lo, dtype):
            prompt = rng.integers(lo, vocab, 128).tolist()
            table = [("t%d " % i).encode() for i in range(vocab)]
            con = KC.Constraint(r"[ -~]*", table)
            t0 = time.perf_counter()
            gram = KC.GrammarConstraint([("s", r"[ -~]*")], table)
            one_rule_ms = (time.perf_counter() - t0) * 1e3
            legs = {
                "greedy_plain": lambda n: dec.generate(prompt, n),
                "greedy_regex": lambda n: dec.generate_constrained(con, prompt, n)[0],
                "greedy_grammar": lambda n: dec.generate_grammar(gram, prompt, n)[0],
                "sampled_plain": lambda n: dec.generate_sampled(prompt, n, sample=True, seed=7, **SAMPLING)[0],
                "sampled_regex": lambda n: dec.generate_constrained(con, prompt, n, sample=True, seed=7, **SAMPLING)[0],
                "sampled_grammar": lambda n: dec.generate_grammar(gram, prompt, n, sample=True, seed=7, **SAMPLING)[0],
            }
            for fn in legs.values():
                fn(8)
            rate = {k: [] for k in legs}
            outs = {}
            for rep in range(2):
                for k, fn in legs.items():
                    dt, out = window(lambda: fn(n_new), lambda: fn(1))
                    assert len(out) == n_new, (k, len(out))
                    rate[k].append((n_new - 1) / dt)
                    outs[k] = out
            assert outs["greedy_plain"] == outs["greedy_grammar"] == outs["greedy_regex"]
            assert outs["sampled_plain"] == outs["sampled_grammar"] == outs["sampled_regex"]
            spread = {k: round(abs(v[0] - v[1]) / med(v), 4) for k, v in rate.items()}
            ratio = {m: round(med(rate[m + "_grammar"]) / med(rate[m + "_regex"]), 4) for m in ("greedy", "sampled")}
            cost_us = {m: round((1.0 / med(rate[m + "_grammar"]) - 1.0 / med(rate[m + "_plain"])) * 1e6, 2) for m in ("greedy", "sampled")}
            regex_cost_us = {m: round((1.0 / med(rate[m + "_regex"]) - 1.0 / med(rate[m + "_plain"])) * 1e6, 2) for m in ("greedy", "sampled")}
            # for information: any JSON value on random weights, over a table of single printable characters and a few words
            chars = [bytes([32 + i % 95]) for i in range(vocab)]
            for i, w in enumerate(("true", "false", "null", "\"a\":", "[1,", "{\"", "\"}", "]]", "},")):
                chars[100 + i] = w.encode()
            t0 = time.perf_counter()
            jv = KC.GrammarConstraint(KC.json_value(), chars)
            jv_new_ms = (time.perf_counter() - t0) * 1e3
            dec.generate_grammar(jv, prompt, 8)
            t0 = time.perf_counter()
            ids, res = dec.generate_grammar(jv, prompt, n_new)
            jv_s = time.perf_counter() - t0
            line = {"metric": f"grammar-constrained decoding, {label}", "unit": "grammar / regex-route tokens per second, greedy",
                    "value": ratio["greedy"], "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"random init, one 128-token prompt, {n_new} generated tokens; the plain loop, the pattern route "
                                           "([ -~]* over an all-ASCII table: nothing masked) and the grammar route (the one-rule grammar of the "
                                           "same language) alternated twice in one process, greedy and sampled (temperature 0.8, top-k 40, "
                                           "top-p 0.9, min-p 0.05, one seed); ids equal (asserted)", "vocab": vocab},
                    "tokens_per_s": {k: {"median": round(med(v), 1), "runs": [round(x, 1) for x in v]} for k, v in rate.items()},
                    "spread_between_alternations": spread, "sampled_grammar_over_regex": ratio["sampled"],
                    "grammar_launches_us_per_step": cost_us, "regex_launches_us_per_step": regex_cost_us,
                    "constructor_ms": {"one_rule": round(one_rule_ms, 1), "json_value": round(jv_new_ms, 1), "vocab": vocab},
                    "json_value_random_weights": {"tokens": len(ids), "seconds": round(jv_s, 4), "complete": res["complete"],
                                                  "violated": res["violated"], "final_depth": res["final_depth"]},
                    "weight_bytes": dec.weight_bytes}
            lines.append(line)
            emit(line)

        d = os.path.join(tmp, "llama-1b-grammar")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, synth.LLAMA_1B["vocab_size"], 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small-grammar")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        dec = kjarni_amd.HipDecoder(gd)
        measure("gpt2-small shape, bf16 weights", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_wide_constraint" in which:
        # Method (as llm_wide and llm_grammar): one process on one box, every leg warmed first (graph capture, lane caches); plain
        # generate_wide at 64 lanes -- the parent's route, the yardstick -- alternates twice with generate_wide_constrained under (a)
        # a pattern that masks nothing ([ -~]* over an all-ASCII table) in every lane and (b) the one-rule grammar of the same
        # language; the ids are asserted equal to the plain run's.  A decode window is a whole call minus the same call cut after
        # its first token, so it holds n_new - 1 lock-step steps.  The spread is what the two alternations of one leg differ by;
        # the per-step cost of the added launches is the difference of a leg's and the plain leg's time per step (a kernel trace of
        # KJARNI_WIDE_CONSTRAINT_STEPS=N steps of one leg, KJARNI_WIDE_CONSTRAINT_LEG=plain|pattern|grammar, names the kernels).  For
        # information: json_value at 64 lanes over single-character tokens on random weights (runs may end early).
        from kjarni_amd import constraints as KC
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        n_new, ctx, W = 128, 512, 64
        trace_steps = int(os.environ.get("KJARNI_WIDE_CONSTRAINT_STEPS", "0"))
        trace_leg = os.environ.get("KJARNI_WIDE_CONSTRAINT_LEG", "grammar")
        out_path = os.path.join(ROOT, "profiles", "llm_wide_constraint_bench.jsonl")
        lines = []
        med = lambda xs: float(np.median(xs))  # noqa: E731

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, vocab, lo, dtype):
            prompts = [rng.integers(lo, vocab, 128).tolist() for _ in range(W)]
            table = [("t%d " % i).encode() for i in range(vocab)]
            con = KC.Constraint(r"[ -~]*", table)
            gram = KC.GrammarConstraint([("s", r"[ -~]*")], table)
            ids_of = lambda got: [g["ids"] for g in got]  # noqa: E731
            legs = {
                "plain": lambda n: dec.generate_wide(prompts, n, lanes=W, lane_context=ctx),
                "pattern": lambda n: ids_of(dec.generate_wide_constrained(prompts, n, [con] * W, lanes=W, lane_context=ctx)),
                "grammar": lambda n: ids_of(dec.generate_wide_constrained(prompts, n, [gram] * W, lanes=W, lane_context=ctx)),
            }
            if trace_steps:  # a short run for rocprofv3 --kernel-trace --stats
                legs[trace_leg](trace_steps + 1)
                return
            for fn in legs.values():
                fn(20)
            rate, ms, outs = {k: [] for k in legs}, {k: [] for k in legs}, {}
            for rep in range(2):
                for k, fn in legs.items():
                    dt, out = window(lambda: fn(n_new), lambda: fn(1))
                    assert all(len(o) == n_new for o in out), k
                    rate[k].append(W * (n_new - 1) / dt)
                    ms[k].append(dt * 1e3 / (n_new - 1))
                    outs[k] = out
            assert outs["plain"] == outs["pattern"] == outs["grammar"]
            spread = {k: round(abs(v[0] - v[1]) / med(v), 4) for k, v in rate.items()}
            chars = [bytes([32 + i % 95]) for i in range(vocab)]
            for i, w in enumerate(("true", "false", "null", "\"a\":", "[1,", "{\"", "\"}", "]]", "},")):
                chars[100 + i] = w.encode()
            jv = KC.GrammarConstraint(KC.json_value(), chars)
            dec.generate_wide_constrained(prompts, 8, [jv] * W, lanes=W, lane_context=ctx)
            t0 = time.perf_counter()
            got = dec.generate_wide_constrained(prompts, n_new, [jv] * W, lanes=W, lane_context=ctx)
            jv_s = time.perf_counter() - t0
            line = {"metric": f"constrained decoding in 64 wide lanes, {label}", "unit": "pattern-route / plain tokens per second at 64 lanes",
                    "value": round(med(rate["pattern"]) / med(rate["plain"]), 4), "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"random init, one 128-token prompt per lane, {n_new} generated tokens per lane, lane_context {ctx}; plain "
                                           "generate_wide, a pattern that masks nothing and the one-rule grammar of the same language in every "
                                           "lane, alternated twice in one process; ids equal (asserted)", "vocab": vocab, "lanes": W},
                    "tokens_per_s": {k: {"median": round(med(v), 1), "runs": [round(x, 1) for x in v]} for k, v in rate.items()},
                    "ms_per_step": {k: {"median": round(med(v), 4), "runs": [round(x, 4) for x in v]} for k, v in ms.items()},
                    "spread_between_alternations": spread,
                    "grammar_over_pattern": round(med(rate["grammar"]) / med(rate["pattern"]), 4),
                    "grammar_over_plain": round(med(rate["grammar"]) / med(rate["plain"]), 4),
                    "added_launches_us_per_step": {k: round((med(ms[k]) - med(ms["plain"])) * 1e3, 2) for k in ("pattern", "grammar")},
                    "json_value_random_weights": {"tokens": sum(len(g["ids"]) for g in got), "seconds": round(jv_s, 4),
                                                  "complete": sum(g["result"]["complete"] for g in got),
                                                  "violated": sum(g["result"]["violated"] for g in got)},
                    "weight_bytes": dec.weight_bytes}
            lines.append(line)
            emit(line)

        d = os.path.join(tmp, "llama-1b-wide-constraint")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, synth.LLAMA_1B["vocab_size"], 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        if not trace_steps:  # (the trace run is the Llama shape alone)
            gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
            gd = os.path.join(tmp, "gpt2-small-wide-constraint")
            gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
            dec = kjarni_amd.HipDecoder(gd)
            measure("gpt2-small shape, bf16 weights", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
            del dec
            with open(out_path, "w") as f:
                for line in lines:
                    f.write(json.dumps(line) + "\n")

    if "llm_qwen3" in which:
        from tests import qwen3_fixture
        geo = dict(qwen3_fixture.Q3_06B_WIDTHS, num_hidden_layers=28, vocab_size=151936, max_position_embeddings=4096, eos_token_id=[])
        d = os.path.join(tmp, "qwen3-0.6b")
        qwen3_fixture.qwen3_model(d, geo, seed=0, store_bf16=True, std=0.02)
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        prompt = np.random.default_rng(0).integers(1000, 100000, 128).tolist()
        trace = int(os.environ.get("KJARNI_QWEN3_TRACE", "0"))
        if trace:
            dec.generate(prompt, trace)
            return
        n_new = 256
        dec.generate(prompt, 8)                                               # warm-up (graph capture)
        runs = []
        for _ in range(3):                                                    # medians of three runs, each ended by a synchronise
            t0 = time.perf_counter()
            dec.reset()
            dec.forward(prompt, fetch=False)
            t_prefill = time.perf_counter() - t0
            t0 = time.perf_counter()
            out = dec.generate(prompt, n_new)
            runs.append((t_prefill, time.perf_counter() - t0 - t_prefill, len(out)))
        t_prefill = float(np.median([r[0] for r in runs]))
        t_dec = float(np.median([r[1] for r in runs]))
        n_out = runs[0][2]
        kv_bytes = 2 * geo["num_hidden_layers"] * geo["num_key_value_heads"] * geo["head_dim"] * 4 * (128 + n_new / 2)
        per_tok = dec.weight_bytes + kv_bytes
        line = {"metric": "tokens/sec greedy decode, Qwen3-0.6B shape, bf16 weights, batch 1", "value": round(n_out / t_dec, 1),
                "unit": "tokens/s", "n_gpus": 1, "dtype": "bf16 weights, f32 activations/accumulate/KV", "data": "synthetic",
                "config": {"workload": "Qwen3-0.6B geometry (1024 hidden, 28 layers, 16/8 heads of 128, intermediate 3072, vocab 151936, tied "
                                       f"head), random init, 128-token prompt, {n_out} generated tokens; medians of 3 runs"},
                "ms_prefill_128": round(t_prefill * 1e3, 2), "ms_per_token": round(t_dec * 1e3 / n_out, 4), "weight_bytes": dec.weight_bytes,
                "launches_per_layer_per_step": 6,
                "runs_ms_per_token": [round(r[1] * 1e3 / r[2], 4) for r in runs],
                "roofline": {"kernel": "llm_gemv kernels (weight stream) + decode_attention_partial", "bound": "hbm",
                             "achieved": round(per_tok * n_out / t_dec / 1e9, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                             "frac": round(per_tok * n_out / t_dec / 1e9 / PEAK_HBM_GBS, 4), "traffic": None,
                             "algorithmic_bytes_per_token": int(per_tok)}}
        emit(line)
        with open(os.path.join(ROOT, "profiles", "qwen3_bench_llm.jsonl"), "w") as f:
            f.write(json.dumps(line) + "\n")
        del dec

    if "llm_logprobs" in which:
        # Method (as llm_constraint): one process on one box, everything warmed first; the same loop with log-probabilities off -- the
        # yardstick -- alternates with top_k 0 and top_k 8, twice, greedy and sampled (the family-neutral config below, one seed); a
        # decode window is a whole generation minus the same call cut after its first token; the ids of the three legs are equal
        # (asserted).  Wide: 64 lanes, one 128-token prompt per lane, 128 new tokens, generate_wide against generate_wide_logprobs
        # at top_k 8.  The kernel pair alone: kjarni_hip_op_token_logprobs_bench over seeded rows at V = 128 256 and 151 936, 1 and
        # 64 rows, against the one-workgroup-per-row score kernel on the same rows 8 at a time (50 repeats between two events).
        # A leg whose two runs differ by more than 10 % of their median goes into "unstable_legs" and its ratio is null.
        from kjarni_amd import ops as KO
        from tests import gpt2_fixture
        rng = np.random.default_rng(0)
        n_new = int(os.environ.get("KJARNI_LOGPROBS_TOKENS", "256"))
        out_path = os.path.join(ROOT, "profiles", "llm_logprobs_bench.jsonl")
        lines = []
        med = lambda xs: float(np.median(xs))  # noqa: E731
        SAMPLING = dict(temperature=0.8, top_p=0.9, min_p=0.05)

        def window(fn_full, fn_first):
            t0 = time.perf_counter()
            fn_first()
            t1 = time.perf_counter()
            out = fn_full()
            t2 = time.perf_counter()
            return (t2 - t1) - (t1 - t0), out

        def measure(label, dec, vocab, lo, dtype):
            prompt = rng.integers(lo, vocab, 128).tolist()
            legs = {
                "greedy_off": lambda n: dec.generate(prompt, n),
                "greedy_k0": lambda n: dec.generate_logprobs(prompt, n, top_k=0)["ids"],
                "greedy_k8": lambda n: dec.generate_logprobs(prompt, n, top_k=8)["ids"],
                "sampled_off": lambda n: dec.generate_sampled(prompt, n, sample=True, seed=7, top_k=40, **SAMPLING)[0],
                "sampled_k0": lambda n: dec.generate_logprobs(prompt, n, top_k=0, sample=True, seed=7, sampling_top_k=40, **SAMPLING)["ids"],
                "sampled_k8": lambda n: dec.generate_logprobs(prompt, n, top_k=8, sample=True, seed=7, sampling_top_k=40, **SAMPLING)["ids"],
            }
            for fn in legs.values():
                fn(8)
            rate = {k: [] for k in legs}
            outs = {}
            for rep in range(2):
                for k, fn in legs.items():
                    dt, out = window(lambda: fn(n_new), lambda: fn(1))
                    assert len(out) == n_new, (k, len(out))
                    rate[k].append((n_new - 1) / dt)
                    outs[k] = out
            assert outs["greedy_off"] == outs["greedy_k0"] == outs["greedy_k8"] and outs["sampled_off"] == outs["sampled_k0"] == outs["sampled_k8"]
            prompts = [rng.integers(lo, vocab, 128).tolist() for _ in range(64)]
            wide = {"wide64_off": lambda n: dec.generate_wide(prompts, n, lanes=64, lane_context=512),
                    "wide64_k8": lambda n: [g["ids"] for g in dec.generate_wide_logprobs(prompts, n, top_k=8, lanes=64, lane_context=512)]}
            for fn in wide.values():
                fn(20)
            wrate = {k: [] for k in wide}
            wouts = {}
            for rep in range(2):
                for k, fn in wide.items():
                    dt, out = window(lambda: fn(128), lambda: fn(1))
                    assert all(len(o) == 128 for o in out), k
                    wrate[k].append(64 * 127 / dt)
                    wouts[k] = out
            assert wouts["wide64_off"] == wouts["wide64_k8"]
            # a leg whose two runs lie more than 10 % of their median apart is no figure: it is listed and its ratio left out
            unstable = sorted(k for k, v in {**rate, **wrate}.items() if (max(v) - min(v)) > 0.10 * med(v))
            ratio = lambda a, b, r=rate: None if a in unstable or b in unstable else round(med(r[a]) / med(r[b]), 4)  # noqa: E731
            line = {"metric": f"generation log-probabilities, {label}", "unit": "top_k 8 / off tokens per second, greedy", "value": ratio("greedy_k8", "greedy_off"),
                    "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"random init, one 128-token prompt, {n_new} generated tokens; log-probabilities off, top_k 0 and top_k 8 "
                                           "alternated twice in one process, greedy and sampled (temperature 0.8, top-k 40, top-p 0.9, min-p 0.05, "
                                           "one seed), ids equal (asserted); 64 wide lanes: one 128-token prompt per lane, 128 tokens, off and top_k 8"},
                    "tokens_per_s": {k: {"median": round(med(v), 1), "runs": [round(x, 1) for x in v]} for k, v in {**rate, **wrate}.items()},
                    "over_off": {"greedy_k0": ratio("greedy_k0", "greedy_off"), "greedy_k8": ratio("greedy_k8", "greedy_off"),
                                 "sampled_k0": ratio("sampled_k0", "sampled_off"), "sampled_k8": ratio("sampled_k8", "sampled_off"),
                                 "wide64_k8": ratio("wide64_k8", "wide64_off", wrate)},
                    "unstable_legs": unstable, "weight_bytes": dec.weight_bytes}
            lines.append(line)
            emit(line)

        d = os.path.join(tmp, "llama-1b-logprobs")
        synth.llm_model(d, synth.LLAMA_1B, seed=0, store_bf16=True, max_position_embeddings=4096, eos_token_id=[])
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        measure("Llama-3.2-1B shape, bf16 weights", dec, synth.LLAMA_1B["vocab_size"], 1000, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        gcfg = gpt2_fixture.gpt2_config(n_embd=768, n_layer=12, n_head=12, n_ctx=1024, vocab_size=50257, eos_token_id=None)
        gd = os.path.join(tmp, "gpt2-small-logprobs")
        gpt2_fixture.gpt2_model(gd, gcfg, seed=0, store_bf16=True, buffers=False, std=0.02)
        dec = kjarni_amd.HipDecoder(gd)
        measure("gpt2-small shape, bf16 weights", dec, 50257, 0, "bf16 weights, f32 activations/accumulate/KV")
        del dec
        for vocab in (128256, 151936):
            for rows in (1, 64):
                x = (rng.standard_normal((rows, vocab)) * 3.0).astype(np.float32)
                KO.token_logprobs_bench(x, 8, 5)
                runs = [KO.token_logprobs_bench(x, 8, 50) for _ in range(3)]
                pair, score = med([r[0] for r in runs]), med([r[1] for r in runs])
                line = {"metric": f"log-probability kernel pair alone, V {vocab}, {rows} row(s)", "unit": "score-rows kernel ms / pair ms",
                        "value": round(score / pair, 3), "n_gpus": 1, "dtype": "f32", "data": "synthetic",
                        "config": {"workload": "seeded normal logits x 3; 50 back-to-back repeats between two events, median of 3; the pair: slab "
                                               "pass + finish, top_k 8; the score-rows kernel: one 256-thread workgroup per row, 8 rows a launch"},
                        "pair_us": round(pair * 1e3, 2), "score_rows_us": round(score * 1e3, 2), "slabs": KO.token_logprob_slabs(rows, vocab),
                        "row_bytes": vocab * 4}
                lines.append(line)
                emit(line)
        with open(out_path, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_embed" in which:
        # Method (measuring guide, section 5): one process on one box; every shape is warmed first; embed() returns after a
        # synchronise and a device-to-host copy, forward(fetch=True) after the copy of its hidden rows; medians.  The packed call and
        # the per-sentence loop over 64 x 128 are alternated twice, three runs each.
        from tests import qwen3_fixture
        geo = dict(qwen3_fixture.Q3_06B_WIDTHS, num_hidden_layers=28, vocab_size=151936, max_position_embeddings=4096, eos_token_id=[])
        d = os.path.join(tmp, "qwen3-0.6b-embed")
        qwen3_fixture.qwen3_model(d, geo, seed=0, store_bf16=True, std=0.02)
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        rng = np.random.default_rng(0)
        dtype = "bf16 weights, f32 activations/accumulate"
        shape = "Qwen3-0.6B geometry (1024 hidden, 28 layers, 16/8 heads of 128, intermediate 3072, vocab 151936), random init"
        lines = []

        def batch(lengths):
            flat = rng.integers(1000, 100000, int(np.sum(lengths))).astype(np.uint32)
            return flat, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)

        def run_ms(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        for label, lengths in (("4096 x 128 tokens", np.full(4096, 128)), ("4096 ragged sentences of U{16..128} tokens", rng.integers(16, 129, 4096))):
            flat, offsets = batch(lengths)
            out = np.zeros((len(lengths), dec.hidden), np.float32)
            dec.embed_flat(flat, offsets, True, out)
            runs = [run_ms(lambda: dec.embed_flat(flat, offsets, True, out)) for _ in range(3)]
            ms = float(np.median(runs))
            first, vec, mfma = kjarni_amd.embed_plan(lengths.tolist(), dec.head_dim)
            line = {"metric": f"sentences/sec decoder embed (last-token pool), Qwen3-0.6B shape, bf16 weights, {label}",
                    "value": round(len(lengths) / ms * 1e3, 1), "unit": "sentences/s", "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"{shape}; HipDecoder.embed of token ids, normalize on; medians of 3 runs after one warm-up"},
                    "tokens": int(np.sum(lengths)), "tokens_per_s": round(float(np.sum(lengths)) / ms * 1e3, 1), "ms": round(ms, 2),
                    "chunks": len(first) - 1, "runs_ms": [round(x, 2) for x in runs]}
            emit(line)
            lines.append(line)
        for n in (1, 8, 64):
            flat, offsets = batch(np.full(n, 128))
            out = np.zeros((n, dec.hidden), np.float32)
            seqs = [flat[offsets[i]:offsets[i + 1]] for i in range(n)]

            def loop():
                for s in seqs:
                    dec.reset()
                    dec.forward(s)
            kinds = {"embed": lambda: dec.embed_flat(flat, offsets, True, out)}
            if n == 64:
                kinds["forward_loop"] = loop
            for fn in kinds.values():
                fn()
            runs = {k: [] for k in kinds}
            for rep in range(2):
                for _ in range(3):
                    for k, fn in kinds.items():
                        runs[k].append(run_ms(fn))
            med = {k: float(np.median(v)) for k, v in runs.items()}
            line = {"metric": f"latency decoder embed, Qwen3-0.6B shape, bf16 weights, {n} x 128 tokens", "value": round(med["embed"], 3),
                    "unit": "ms", "n_gpus": 1, "dtype": dtype, "data": "synthetic",
                    "config": {"workload": f"{shape}; alternated twice in one process, medians of 6 runs, every run ends in a synchronise"},
                    "sentences": n, "embed_ms": round(med["embed"], 3), "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
            if n == 64:
                line["forward_loop_ms"] = round(med["forward_loop"], 3)
                line["forward_loop_over_embed"] = round(med["forward_loop"] / med["embed"], 2)
            emit(line)
            lines.append(line)
        dec.reset()
        del dec
        with open(os.path.join(ROOT, "profiles", "decoder_embed_bench.jsonl"), "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    if "llm_rerank" in which:
        # Method (measuring guide, section 5; as llm_score_batch): one process on one box; every leg of a case is warmed first,
        # then the legs are alternated twice, two runs each; every run ends in a synchronise (answer_logits() returns after one,
        # forward(fetch=True) after the copy of its logits); medians over the 4 runs of a leg.  The forward() loop over the same
        # sequences is what there was before answer_logits().
        from tests import qwen3_fixture
        geo = dict(qwen3_fixture.Q3_06B_WIDTHS, num_hidden_layers=28, vocab_size=151936, max_position_embeddings=4096, eos_token_id=[])
        d = os.path.join(tmp, "qwen3-0.6b-rerank")
        qwen3_fixture.qwen3_model(d, geo, seed=0, store_bf16=True, std=0.02)
        dec = kjarni_amd.HipDecoder(d, max_context=2048)
        rng = np.random.default_rng(0)
        dtype = "bf16 weights, f32 activations/accumulate"
        shape = "Qwen3-0.6B geometry (1024 hidden, 28 layers, 16/8 heads of 128, intermediate 3072, vocab 151936), random init"
        method = "legs alternated twice in one process, medians of 4 runs, every run ends in a synchronise"
        targets = np.array([9693, 2152], np.uint32)
        lines = []
        for n in (16, 64, 256):     # one query of 64 tokens in front of n documents of 128
            query = rng.integers(1000, 100000, 64).astype(np.uint32)
            shared = [np.concatenate([query, rng.integers(1000, 100000, 128).astype(np.uint32)]) for _ in range(n)]
            distinct = [s.copy() for s in shared]
            for i, s in enumerate(distinct):
                s[0] = 100 + i                                                  # (same shapes, nothing shared)
            off = np.concatenate([[0], np.cumsum([len(s) for s in shared])]).astype(np.int32)
            fs, fd = np.concatenate(shared), np.concatenate(distinct)

            def loop():
                for s in shared:
                    dec.reset()
                    dec.forward(s)
            legs = {"shared": lambda: dec.answer_logits_flat(fs, off, targets), "not_shared": lambda: dec.answer_logits_flat(fd, off, targets),
                    "forward_loop": loop}
            r0 = dec.answer_rows()
            legs["shared"]()
            r1 = dec.answer_rows()
            legs["not_shared"]()
            r2 = dec.answer_rows()
            legs["forward_loop"]()
            runs = {k: [] for k in legs}
            for rep in range(2):
                for _ in range(2):
                    for k, fn in legs.items():
                        t0 = time.perf_counter()
                        fn()
                        runs[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in runs.items()}
            line = {"metric": f"forward loop / answer_logits, Qwen3-0.6B shape, bf16 weights, a 64-token query x {n} documents of 128 tokens",
                    "value": round(med["forward_loop"] / med["shared"], 2), "unit": "ratio of medians", "n_gpus": 1, "dtype": dtype,
                    "data": "synthetic", "config": {"workload": f"{shape}; {method}; not_shared: every sequence's token 0 made distinct"},
                    "documents": n, "shared_ms": round(med["shared"], 3), "not_shared_ms": round(med["not_shared"], 3),
                    "forward_loop_ms": round(med["forward_loop"], 3), "not_shared_over_shared": round(med["not_shared"] / med["shared"], 3),
                    "documents_per_s": round(n / med["shared"] * 1e3, 1), "rows_shared": r1[0] - r0[0], "rows_saved_shared": r1[1] - r0[1],
                    "rows_not_shared": r2[0] - r1[0], "rows_saved_not_shared": r2[1] - r1[1],
                    "runs": {k: [round(x, 3) for x in v] for k, v in runs.items()}}
            emit(line)
            lines.append(line)
        dec.reset()
        del dec
        with open(os.path.join(ROOT, "profiles", "decoder_rerank_bench.jsonl"), "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
