"""Cases shared by the draft-model tests (tests/test_draft_model_host.py, tests/test_gpu_draft_model.py): the per-round
(drafted, accepted) log a greedy run with a drafter implies, and drafter oracles to feed it.  Nothing here touches the GPU.

A drafter oracle is a callable (history, k) -> (tokens, gap): the drafter's greedy continuation of `history` by k tokens
and the smallest gap between its two best logits over those k decisions (inf for a table-driven oracle)."""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import numpy as np

DrafterOracle = Callable[[Sequence[int], int], Tuple[List[int], float]]


def simulate(target_out: Sequence[int], drafter_oracle: DrafterOracle, prompt: Sequence[int], k: int) -> Tuple[List[Tuple[int, int]], float]:
    """The (m, a) of every verify round of a draft-model run whose output is target_out, and the smallest drafter gap met.
    The first token comes from the prompt's logits; each round then drafts m = k tokens after the history and accepts the a
    that agree with the output, emitting a + 1.  The last entry's a is a lower bound when the output ends inside its draft."""
    out = list(target_out)
    if not out:
        return [], float("inf")
    T, pos, log, gap = list(prompt) + out[:1], 1, [], float("inf")
    while pos < len(out):
        draft, g = drafter_oracle(T, k)
        assert len(draft) == k
        gap = min(gap, g)
        a = 0
        while a < k and pos + a < len(out) and draft[a] == out[pos + a]:
            a += 1
        log.append((k, a))
        T += out[pos:pos + a + 1]
        pos += a + 1
    return log, gap


def table_drafter(sequence: Sequence[int], wrong_at: Sequence[int] = (), offset: int = 1000) -> DrafterOracle:
    """A drafter that continues any history with sequence[len(history):] (padded with its last id), except that the tokens
    at the absolute positions in wrong_at are replaced by id + offset."""
    seq, wrong = list(sequence), set(wrong_at)

    def oracle(history, k):
        n = len(history)
        toks = []
        for i in range(n, n + k):
            t = seq[i] if i < len(seq) else seq[-1]
            toks.append(t + offset if i in wrong else t)
        return toks, float("inf")
    return oracle


class ModelDrafter:
    """A drafter oracle over a model with new() -> cache and logits(ids, cache) -> [len(ids), vocab] (appending to the
    cache), greedy with the last maximum winning.  Keeps the cache of the longest prefix it shares with the call before."""

    def __init__(self, model, truncate: Callable):
        self.model, self.truncate, self.tokens, self.cache = model, truncate, [], model.new()

    def __call__(self, history, k):
        history = list(history)
        keep = 0
        while keep < min(len(self.tokens), len(history) - 1) and self.tokens[keep] == history[keep]:
            keep += 1
        self.cache = self.truncate(self.cache, keep)
        row = self.model.logits(history[keep:], self.cache)[-1]
        self.tokens = list(history)
        toks, gap = [], float("inf")
        for i in range(k):
            top = np.partition(np.asarray(row, np.float64), -2)[-2:]
            gap = min(gap, float(top[1] - top[0]))
            toks.append(int(len(row) - 1 - np.argmax(row[::-1])))
            if i + 1 < k:
                row = self.model.logits([toks[-1]], self.cache)[-1]
                self.tokens.append(toks[-1])
        return toks, gap
