"""The float64 rule of generation log-probabilities (kjarni_hip_decoder_generate_logprobs and its kin), with no GPU in it.

A record belongs to one emitted token: the log-softmax of the step's RAW logits row (as the vocabulary head wrote it: before any
mask, processor, temperature or cut) at the emitted id, and the top_k largest entries of that row in score_topk's order --
descending value, among equal values the larger id first, +0.0 == -0.0, NaN lowest."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

TOPK_MAX = 8
GRID_TARGET, MIN_SLAB, MAX_SLABS = 512, 1024, 64


def slabs(rows: int, vocab: int) -> int:
    """The slab rule of the kernels, restated: min(64, ceil(vocab / 1024), max(1, ceil(512 / rows))) slabs, the slab length
    rounded up to a multiple of 4, the slabs recounted over that length."""
    want = min(MAX_SLABS, -(-vocab // MIN_SLAB), max(1, -(-GRID_TARGET // rows)))
    length = -(-(-(-vocab // want)) // 4) * 4
    return -(-vocab // length)


def slab_len(rows: int, vocab: int) -> int:
    want = min(MAX_SLABS, -(-vocab // MIN_SLAB), max(1, -(-GRID_TARGET // rows)))
    return -(-(-(-vocab // want)) // 4) * 4


def lse64(row) -> float:
    x = np.asarray(row, np.float64)
    mx = x.max()
    return float(mx + np.log(np.exp(x - mx).sum()))


def log_softmax64(row) -> np.ndarray:
    x = np.asarray(row, np.float64)
    return x - lse64(x)


def topk_ids(row, k: int) -> np.ndarray:
    """The ids of the k largest entries: descending value, among equal values the larger id first; the two zeros are one value;
    NaN sorts below everything."""
    x = np.asarray(row, np.float64).copy()
    x[x == 0.0] = 0.0                       # -0.0 -> +0.0
    x[np.isnan(x)] = -np.inf                # lowest (rows with both NaN and -inf are not part of any case)
    ids = np.arange(x.size)
    order = np.lexsort((-ids, -x))          # primary: value descending; secondary: id descending
    return order[:k].astype(np.int64)


def record(row, token: int, k: int) -> Dict[str, object]:
    """{logprob, topk_ids [k], topk_logprob [k], lse} of one raw row and its emitted token."""
    lsm = log_softmax64(row)
    ids = topk_ids(row, k)
    return {"logprob": float(lsm[token]), "topk_ids": ids, "topk_logprob": lsm[ids], "lse": lse64(row)}


def run_record(raw_rows: Sequence[np.ndarray], ids: Sequence[int], k: int) -> Dict[str, np.ndarray]:
    """The records of a run: raw_rows[i] is the raw logits row token ids[i] was decided from."""
    assert len(raw_rows) >= len(ids)
    recs = [record(raw_rows[i], int(t), k) for i, t in enumerate(ids)]
    return {"logprob": np.array([r["logprob"] for r in recs], np.float64),
            "topk_ids": np.array([r["topk_ids"] for r in recs], np.int64).reshape(len(ids), k),
            "topk_logprob": np.array([r["topk_logprob"] for r in recs], np.float64).reshape(len(ids), k),
            "lse": np.array([r["lse"] for r in recs], np.float64)}


def clear_slots(row, k: int, gap: float) -> np.ndarray:
    """bool [k]: slot j's id is decided by more than rounding -- the sorted values j - 1, j, j + 1 are at least `gap` apart
    (an exact tie is decided by the tie rule, but only where the compared rows are the same bits: the caller's business)."""
    x = np.sort(np.asarray(row, np.float64))[::-1][:k + 1]
    d = x[:-1] - x[1:] if x.size > 1 else np.array([])
    ok = np.ones(k, bool)
    for j in range(k):
        if j > 0 and d[j - 1] < gap:
            ok[j] = False
        if j < d.size and d[j] < gap:
            ok[j] = False
    return ok


class Qwen3Logits:
    """tests/qwen3_ref64.Qwen3Ref64 (or the MoE reference) behind the new() / logits(ids, cache) interface of the other wrappers."""

    def __init__(self, ref, cfg):
        self.ref, self.vocab, self.first_id = ref, cfg["vocab_size"], 4

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        return self.ref.logits(self.ref.forward(list(ids), cache))


def greedy_trace(ref, prompt: Sequence[int], n: int, stops: Sequence[int] = ()) -> Dict[str, object]:
    """n greedy steps of a float64 reference with `new()` / `logits(ids, cache)` (tests/test_gpu_lookup.py's wrappers): the raw
    row of every step, the picks (last maximum wins), stopping before a stop id."""
    cache = ref.new()
    row = ref.logits(list(prompt), cache)[-1]
    rows: List[np.ndarray] = []
    out: List[int] = []
    for _ in range(n):
        rows.append(np.asarray(row, np.float64))
        t = int(len(row) - 1 - np.argmax(row[::-1]))
        if t in stops:
            break
        out.append(t)
        row = ref.logits([t], cache)[-1]
    return {"rows": rows, "ids": out}
