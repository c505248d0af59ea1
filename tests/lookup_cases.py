"""Cases shared by the prompt-lookup tests (tests/test_lookup_host.py, tests/test_gpu_lookup.py): the draft rule, the
seeded histories both implementations are checked on, and the per-step (drafted, accepted) log a greedy run implies.
Nothing here touches the GPU."""
from __future__ import annotations

from typing import Iterator, List, Sequence, Tuple

import numpy as np

DEFAULT = (7, 3, 1)   # draft_tokens, ngram_max, ngram_min
# every (draft_tokens, ngram_max, ngram_min) the interface accepts: 7 x 10
CONFIGS = [(D, hi, lo) for D in range(1, 8) for hi in range(1, 5) for lo in range(1, hi + 1)]


def lookup_draft(T: Sequence[int], ngram_max: int, ngram_min: int, D: int) -> List[int]:
    """The normative rule.  T is the history; its last element is the token that is not in the cache yet."""
    n, best = len(T), None
    for e in range(1, n):                      # a continuation would start at T[e]
        m = 0                                  # length of the match that ends just before e, against the suffix of T
        while m < ngram_max and e - 1 - m >= 0 and T[e - 1 - m] == T[n - 1 - m]:
            m += 1
        if m < ngram_min:
            continue
        key = (m, min(D, n - e), e)            # longest match, then longest continuation, then latest
        if best is None or key > best:
            best = key
    return [] if best is None else list(T[best[2]:best[2] + best[1]])


def histories(count: int = 2000, seed: int = 20) -> Iterator[Tuple[List[int], Tuple[int, int, int]]]:
    """`count` seeded histories, lengths 1..300 over alphabets of 2..50 ids, cycling through every config."""
    rng = np.random.default_rng(seed)
    for i in range(count):
        n, alphabet = int(rng.integers(1, 301)), int(rng.integers(2, 51))
        yield rng.integers(0, alphabet, n).tolist(), CONFIGS[i % len(CONFIGS)]


EDGE_CASES = [
    ("n = 1", [5], DEFAULT),
    ("all tokens equal", [9] * 40, DEFAULT),
    ("all tokens equal, short", [9, 9], DEFAULT),
    ("no match", list(range(30)), DEFAULT),
    ("the only match at e = 1", [3, 1, 2, 4, 5, 3], DEFAULT),
    ("ngram_min longer than any match", [1, 2, 3, 9, 2, 3], (7, 4, 3)),
    ("ngram_min met exactly", [1, 2, 3, 9, 1, 2, 3], (7, 4, 3)),
    ("longest continuation beats latest", [1, 2, 1, 2, 1, 2, 1, 2, 1], (7, 1, 1)),
    ("longer match beats longer continuation", [7, 8, 1, 2, 3, 4, 5, 6, 8, 9, 7, 8], (7, 3, 1)),
]


def simulate(prompt: Sequence[int], oracle_out: Sequence[int], cfg=DEFAULT) -> List[Tuple[int, int]]:
    """The (m, a) of every verify step of a lookup run whose greedy output is oracle_out: the first token comes from the
    prompt's logits, then each step drafts m tokens from the history and accepts the a that agree with the output, emitting
    a + 1.  The last entry's a is a lower bound when the output ends inside its draft."""
    D, ngram_max, ngram_min = cfg
    out = list(oracle_out)
    if not out:
        return []
    T, pos, log = list(prompt) + out[:1], 1, []
    while pos < len(out):
        draft = lookup_draft(T, ngram_max, ngram_min, D)
        a = 0
        while a < len(draft) and pos + a < len(out) and draft[a] == out[pos + a]:
            a += 1
        log.append((len(draft), a))
        T += out[pos:pos + a + 1]
        pos += a + 1
    return log
