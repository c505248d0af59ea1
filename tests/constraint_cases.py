"""Constrained decoding restated in Python, shared by tests/test_constraint_host.py and tests/test_gpu_constraint.py: walks of
an exported DFA table, the token mask by a numpy walk vectorised by byte position, token tables for the tiny test models, and the
float64 oracle of a constrained run (tests/llm_ref64.py through tests/sampled_lookup_cases.py, with the mask applied in Python).
Nothing here touches the GPU."""
from __future__ import annotations

import itertools
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import sampled_lookup_cases as SC

DEAD = 0xFFFF
GAP = SC.GAP

# pattern -> the alphabet its strings are enumerated over (tests/test_constraint_host.py); together they cover every item of the
# syntax: literals, non-ASCII literals, every escape, \d \w \s, `.`, classes, negated classes, both groups, alternation, every
# quantifier form.  "é" (2 bytes) and "€" (3 bytes) are the non-ASCII characters.
PATTERNS: Dict[str, str] = {
    r"a(b|c)*d": "abcd",
    r"(?:ab|a)(?:c|bc)?": "abc",
    r"a+b?c*": "abc",
    r"a{2}b{1,}c{0,2}": "abc",
    r"(?:a{2,3}|b){1,2}": "ab",
    r"\d+\.\d{1,2}": "01.a",
    r"\w\s\w": "a_ 0\t-",
    r".a.": "a\nbé",
    r"[^a\n]{1,3}b": "ab\né",
    r"[a-c0-1_]*x": "ac1_x-",
    r"é€?[ab]": "é€ab",
    r"\\\.\n\t\r\"\x41\{\}\[\]\(\)\|\*\+\?": "\\.\n\t\r\"A{}[]()|*+?",
    r"[\\\]\-x]{2}": "\\]-xa",
    r"\xe9|\x7e\x21": "é~!a",
    r"(|a)(b|)": "ab",
    r"-?(?:0|[1-9][0-9]*)": "-019",
}
MAX_LEN = {p: 6 for p in PATTERNS}
MAX_LEN[r"\\\.\n\t\r\"\x41\{\}\[\]\(\)\|\*\+\?"] = 0   # one string only: checked by itself, not by enumeration


def strings(alphabet: str, max_len: int):
    for n in range(max_len + 1):
        for tup in itertools.product(alphabet, repeat=n):
            yield "".join(tup)


def walk(trans: np.ndarray, q: int, data: bytes) -> int:
    """The state after `data` from q on an exported table [S, 256]; DEAD when the walk dies."""
    for b in data:
        if q == DEAD:
            return DEAD
        q = int(trans[q, b])
    return q


def flags_by_search(trans: np.ndarray, accepting: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(co-reachable, closed) recomputed from the table: which states reach an accepting state, and which accepting states have
    no outgoing byte."""
    S = trans.shape[0]
    live = accepting.astype(bool).copy()
    changed = True
    while changed:
        changed = False
        for q in range(S):
            if not live[q] and any(t != DEAD and live[t] for t in trans[q]):
                live[q] = changed = True
    closed = np.array([bool(accepting[q]) and bool((trans[q] == DEAD).all()) for q in range(S)])
    return live, closed


# ---- token tables ----------------------------------------------------------------------------------------------------------------

def table(tokens: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    off = np.zeros(len(tokens) + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in tokens], dtype=np.uint64)
    return off, np.frombuffer(b"".join(tokens), np.uint8).copy()


WORDS = ["yes", "no", "maybe", "ye", "es", "ma", "yb", "be", "ay", "ab", "abc", "bcd", "cd", "12", "123", "00", "01", "-1", "-0", "1.5", ".5",
         "e-", "\"a", "a\"", "\":", "{\"", "\"}", "\",\"", "a\":", "{\"a\":", "é", "aé", "€", "\n", "a\n"]


def model_tokens(vocab: int, specials: Sequence[int] = (0, 1, 2, 3), seed: int = 0) -> List[bytes]:
    """A token table for a tiny test model: the ids in `specials` have no bytes; then every character of a small alphabet, a list
    of words that make the test patterns reachable in more than one way, one 40-byte token, and seeded strings of 2..4 characters."""
    alphabet = "abcdemnosy0123456789-.\"{}:, "
    rng = np.random.default_rng(seed)
    pool = [c.encode() for c in alphabet] + [w.encode() for w in WORDS] + [b"ab" * 20]
    out: List[bytes] = []
    for i in range(vocab):
        if i in specials:
            out.append(b"")
        elif pool:
            out.append(pool.pop(0))
        else:
            out.append("".join(alphabet[j] for j in rng.integers(0, len(alphabet), int(rng.integers(2, 5)))).encode())
    return out


def universal_tokens(vocab: int, stop: int) -> List[bytes]:
    """Every token has (valid UTF-8) bytes except `stop`: under the pattern (.|\\n)* nothing but the stop rule is masked."""
    return [b"" if i == stop else ("t%d " % i).encode() for i in range(vocab)]


# ---- the mask ----------------------------------------------------------------------------------------------------------------------

def allowed_matrix(trans: np.ndarray, tokens: Sequence[bytes]) -> np.ndarray:
    """allowed[q, t]: token t has at least one byte and its walk from q never dies.  One numpy step per byte position."""
    S, V = trans.shape[0], len(tokens)
    ext = np.vstack([trans.astype(np.int32), np.full((1, 256), DEAD, np.int32)])   # row S: the dead state stays dead
    lens = np.array([len(t) for t in tokens], np.int64)
    width = int(lens.max(initial=0))
    padded = np.zeros((V, max(width, 1)), np.uint8)
    for i, t in enumerate(tokens):
        padded[i, :len(t)] = np.frombuffer(t, np.uint8)
    cur = np.repeat(np.arange(S, dtype=np.int32)[:, None], V, axis=1)
    for pos in range(width):
        idx = np.flatnonzero(lens > pos)
        c = cur[:, idx]
        c = np.where(c == DEAD, S, c)
        cur[:, idx] = ext[c, padded[idx, pos][None, :]]
    return (cur != DEAD) & (lens > 0)[None, :]


def pack(allowed: np.ndarray) -> np.ndarray:
    """[S, V] bools as [S, ceil(V / 64)] 64-bit words, bit t % 64 of word t // 64; the tail bits are 0."""
    S, V = allowed.shape
    W = (V + 63) // 64
    bits = np.zeros((S, W * 64), np.uint8)
    bits[:, :V] = allowed
    packed = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little"))   # byte t // 8 holds bit t % 8
    return packed.view("<u8").reshape(S, W).astype(np.uint64)


def unpack(words: np.ndarray, V: int) -> np.ndarray:
    S, W = words.shape
    out = np.zeros((S, W * 64), bool)
    for b in range(64):
        out[:, b::64] = (words >> np.uint64(b)) & np.uint64(1)
    return out


# ---- the host automaton of a run ---------------------------------------------------------------------------------------------------

class HostConstraint:
    """The exported table, the token bytes and a call's stop ids: what the loops' masking and stepping amount to."""

    def __init__(self, regex, tokens: Sequence[bytes], stops: Sequence[int]):
        self.trans, self.accepting, self.closed, self.start = regex.trans, regex.accepting, regex.closed, regex.start
        self.tokens, self.stops = list(tokens), list(stops)
        self.allowed = allowed_matrix(self.trans, self.tokens)

    def legal(self, q: int) -> np.ndarray:
        """The tokens whose logits survive in state q: the mask, with every stop id governed by the accepting rule alone."""
        ok = self.allowed[q].copy()
        for s in self.stops:
            if 0 <= s < ok.size:
                ok[s] = bool(self.accepting[q])
        return ok

    def step(self, q: int, tok: int) -> int:
        return walk(self.trans, q, self.tokens[tok])

    def text(self, ids: Sequence[int]) -> bytes:
        return b"".join(self.tokens[i] for i in ids)

    def live_prefix(self, ids: Sequence[int]) -> bool:
        return walk(self.trans, self.start, self.text(ids)) != DEAD


def _last_max(row: np.ndarray) -> int:
    return int(len(row) - 1 - np.argmax(row[::-1]))


def oracle_run(ref, prompt: Sequence[int], n_new: int, hc: HostConstraint, penalty: float = 1.0, params: Optional[dict] = None,
               uniforms: Optional[Sequence[float]] = None, seed: int = 0, context: int = 0):
    """The constrained loop on the float64 model: mask, then the repetition penalty, then the pick (greedy: the last maximum;
    params given: SC.distribution and a draw).  With params and no uniforms the draws are made here, each in the middle of the
    interval of a seeded choice among the tokens that can be steered to (SC.steer).  Returns (ids, info): info has the draws, the
    final state, complete, and `clear`: whether every decision cleared the float bar -- greedy: the two best surviving logits at
    least GAP * P apart; sampled: every filter decision and every draw with the margins of SC."""
    rng = np.random.default_rng(seed)
    hist, out, draws = list(prompt), [], []
    cache = ref.new()
    row = ref.logits(hist, cache)[-1]
    q, complete, clear = hc.start, False, True
    while len(out) < n_new and (not context or len(hist) < context):
        masked = np.where(hc.legal(q), row, -np.inf)
        P = SC.penalty_factor(hist, penalty)
        proc = SC.penalise(masked, hist, penalty)
        if params is None:
            top = np.sort(proc[np.isfinite(proc)])[-2:]
            if top.size == 2 and top[1] - top[0] < GAP * P:
                clear = False
            tok = _last_max(proc)
        else:
            ids, probs, slack = SC.distribution(proc, P=P, **params)
            M = SC.u_margin(P, params.get("temperature", 1.0))
            if uniforms is None:
                cands = [int(t) for t in ids if SC.steer(ids, probs, int(t), M) is not None]
                if not cands:
                    clear = False
                    cands = [int(ids[np.argmax(probs)])]
                t = cands[int(rng.integers(0, len(cands)))]
                u = SC.steer(ids, probs, t, M)
                u = float(np.float32(np.cumsum(probs)[list(ids).index(t)] - probs[list(ids).index(t)] / 2)) if u is None else u
            else:
                u = float(uniforms[len(draws)])
            draws.append(u)
            if slack < 1.0 or SC.draw_clearance(probs, u) < M:
                clear = False
            tok = SC.pick(ids, probs, u)
        if tok in hc.stops:
            complete = True
            break
        q = hc.step(q, tok)
        assert q != DEAD, "the oracle picked a masked token"
        hist.append(tok)
        out.append(tok)
        if hc.closed[q]:
            complete = True
            break
        if context and len(hist) >= context:
            break
        row = ref.logits([tok], cache)[-1]
    return out, dict(uniforms=draws, final_state=q, complete=complete, accepted=bool(hc.accepting[q]), clear=clear)


def fullmatch(pattern: str, data: bytes) -> bool:
    try:
        return re.fullmatch(pattern, data.decode("utf-8"), re.ASCII) is not None
    except UnicodeDecodeError:
        return False
