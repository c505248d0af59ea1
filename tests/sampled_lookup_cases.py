"""Cases shared by the sampled prompt-lookup tests (tests/test_sampled_lookup_host.py, tests/test_gpu_sampled_lookup.py): the
float64 sampled oracle over the reference models (tests/llm_ref64.py, tests/gpt2_ref64.py), and the preconditions that make
"the same ids as the oracle" a fair demand of an f32 implementation.  Nothing here touches the GPU.

The decoder's float bar is BAR = 1e-4 on logits; GAP = 1e-3 (lanes_cases.GAP) is ten times that.  P is the largest penalty
factor applied to any logit of a row (1 without a penalty): a processed logit is off by at most BAR * P.  A logit error e moves
any cumulative probability of softmax(logits / T) by at most 2 e / T, so
  * every draw sits at least U_MARGIN = 10 * 2 * BAR * P / T away from every boundary of the oracle's cumulative distribution;
  * every filter decision that shapes the outcome clears its boundary by GAP * P in logits (the k-th against the (k + 1)-th
    logit, the survivors against the min-p threshold max + ln(min_p)) or by U_MARGIN in mass (the top-p crossing): see
    distribution() for which decisions those are and why.
Draws are steered: u is the middle of a chosen token's interval, which makes a verify step accept or reject a drafted token on
purpose.  A state whose filters do not clear their boundaries cannot be mended by another draw, so the builder looks one token
ahead and steers to a token whose successor state is clear; every time it has to leave its first choice counts as a redraw, and
at most 1 draw in 4 may be one (more means the margins are wrong for these inputs, not that the inputs are unlucky)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests import lanes_cases as LC
from tests import llm_ref64
from tests import lookup_cases as LK
from tests.gpt2_ref64 import Gpt2Ref64

F32, F64 = np.float32, np.float64
BAR, GAP = 1e-4, LC.GAP
MAX_REDRAW_RATE = 0.25

# model_default_generation_config (chat.cpp) by family: what a Chat / Generator user samples with
FAMILY_DEFAULTS = {
    "gpt2": dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.1, repetition_penalty=1.0),
    "llama": dict(temperature=0.6, top_k=None, top_p=0.9, min_p=0.05, repetition_penalty=1.0),
    "qwen2": dict(temperature=0.7, top_k=40, top_p=0.8, min_p=0.05, repetition_penalty=1.1),
    "mistral": dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05, repetition_penalty=1.15),
}


# ---- float64 models with every row's logits -------------------------------------------------------------------------------------

class Llama64:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = llm_ref64.Ref64(t, cfg), cfg["vocab_size"], 4
        tied = cfg.get("tie_word_embeddings", cfg["model_type"] == "llama") or "lm_head.weight" not in t
        self.head = self.ref.t["model.embed_tokens.weight" if tied else "lm_head.weight"]

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        """Appends ids to the cache; the logits of every new row [len(ids), vocab]."""
        h = self.ref.forward(list(ids), cache)
        return self.ref.rms_norm(h, self.ref.t["model.norm.weight"]) @ self.head.T


class Gpt264:
    def __init__(self, t, cfg):
        self.ref, self.vocab, self.first_id = Gpt2Ref64(t, cfg), cfg["vocab_size"], 0

    def new(self):
        return self.ref.new_cache()

    def logits(self, ids, cache):
        hidden, _ = self.ref.forward(list(ids), cache)
        return hidden @ self.ref.t["wte.weight"].T


# ---- the sampler in float64 -------------------------------------------------------------------------------------------------------

def penalty_factor(history: Sequence[int], penalty: float) -> float:
    """P: the largest factor the repetition penalty applies to any logit for this history."""
    if penalty == 1.0 or not len(history):
        return 1.0
    _, counts = np.unique(np.asarray(history, np.int64), return_counts=True)
    return float(max(penalty, 1.0 / penalty) ** int(counts.max()))


def u_margin(P: float, temperature: float) -> float:
    return 10.0 * 2.0 * BAR * P / temperature


def penalise(row: np.ndarray, history: Sequence[int], penalty: float) -> np.ndarray:
    """apply_repetition_penalty in the arithmetic of `row`'s dtype (float64: the oracle; float32: bit-exact with the host's)."""
    out = np.array(row, copy=True)
    if penalty == 1.0:
        return out
    pen = out.dtype.type(penalty)
    for t in history:
        if 0 <= t < out.size:
            out[t] = out[t] * pen if out[t] < 0 else out[t] / pen
    return out


def _softmax(v):
    e = np.exp(v - v.max())
    return e / e.sum()


def distribution(row: np.ndarray, temperature=1.0, top_k=None, top_p=None, min_p=None, P: float = 1.0, **_):
    """sample_token's distribution (top-k -> top-p -> min-p -> temperature -> softmax) of one processed row in float64:
    (ids ascending, probs, slack); slack >= 1 iff the filter decisions that shape the outcome clear their boundaries (the
    smallest ratio clearance / required clearance; inf when nothing is filtered).

    Each of the three filters keeps a prefix of the same order (logit descending, then position): the k best; through the token
    that carries the mass past top_p (the mass normalised over the k best); the tokens at or above max + ln(min_p) -- p_i >=
    min_p * p_max is that, whatever set normalises p.  The survivors are the shortest prefix, L tokens.  An error of BAR * P per
    logit leaves that set alone when
      (1) the last kept and the first dropped logit are GAP * P apart (no swap at the boundary; the top-k decision when k = L);
      (2) the last kept logit is GAP * P above the min-p threshold, and the first dropped one GAP * P below it when min-p is
          what ends the prefix at L;
      (3) the mass in front of the last kept token is U_MARGIN short of top_p (top-p still reaches it), and the mass through
          it U_MARGIN past top_p when top-p is what ends the prefix at L.
    A decision between two tokens that a later filter drops anyway (the 40th against the 41st logit when min-p keeps nine) has
    no bearing on the outcome and is not among them."""
    v = np.asarray(row, F64)
    V = v.size
    order = np.lexsort((np.arange(V), -v))                                # value descending, then position ascending
    vs = v[order]
    gap, M = GAP * P, u_margin(P, temperature)
    kk = top_k if top_k is not None and top_k < V else V
    thr = vs[0] + np.log(min_p) if min_p is not None and min_p > 0.0 else -np.inf
    n_minp = int(np.count_nonzero(vs >= thr))
    cum, cut = None, kk - 1
    if top_p is not None:
        cum = np.cumsum(_softmax(vs[:kk]))
        over = np.flatnonzero(cum > top_p)
        cut = int(over[0]) if over.size else kk - 1
    L = min(kk, n_minp, cut + 1)
    slack = float("inf")
    if L < V:
        slack = min(slack, float(vs[L - 1] - vs[L]) / gap)                                   # (1)
    if np.isfinite(thr):
        slack = min(slack, float(vs[L - 1] - thr) / gap)                                     # (2)
        if n_minp == L and L < V:
            slack = min(slack, float(thr - vs[L]) / gap)
    if cum is not None:
        if L >= 2:
            slack = min(slack, float(top_p - cum[L - 2]) / M)                                # (3)
        if cut + 1 == L and cum[L - 1] > top_p:
            slack = min(slack, float(cum[L - 1] - top_p) / M)
    idx = np.sort(order[:L])
    t = 1.0 if temperature < 1e-5 else temperature
    return idx, _softmax(v[idx] / t), slack


def pick(ids, probs, u: float) -> int:
    """sample_from_probs: the first id whose running sum reaches u."""
    if u <= 0.0:
        return 0
    cum = np.cumsum(probs)
    hit = np.flatnonzero(cum >= u)
    return int(ids[hit[0]]) if hit.size else -1


def draw_clearance(probs, u: float) -> float:
    """The distance of u from the nearest boundary of the cumulative distribution (the last boundary, 1, is none: past it the
    last token is taken anyway)."""
    cum = np.cumsum(probs)[:-1]
    return float(min(np.abs(cum - u).min(initial=float("inf")), u))


def steer(ids, probs, token: int, M: float) -> Optional[float]:
    """The float32 draw in the middle of `token`'s interval, or None when the interval is narrower than 2.1 * M."""
    j = np.flatnonzero(ids == token)
    if not j.size or probs[j[0]] < 2.1 * M:
        return None
    cum = np.cumsum(probs)
    u = float(F32(cum[j[0]] - probs[j[0]] / 2.0))
    return u if pick(ids, probs, u) == token and draw_clearance(probs, u) >= M else None


# ---- traces -----------------------------------------------------------------------------------------------------------------------

class Trace:
    def __init__(self):
        self.ids: List[int] = []            # the tokens the oracle emits
        self.uniforms: List[float] = []     # the draw that decided each
        self.steps: List[Tuple[int, int]] = []   # (drafted, accepted) of every verify step of a lookup run
        self.rows: List[int] = []           # the row of its step at which each token (after the first) was decided
        self.redraws = 0                    # draws that could not follow the builder's first choice
        self.min_slack = float("inf")       # the tightest filter decision met (>= 1: clear)
        self.min_clear = float("inf")       # the tightest draw, in units of its U_MARGIN (>= 1: clear)
        self.max_P = 1.0


def build_trace(ref, prompt: Sequence[int], n_new: int, params: Dict, lookup=LK.DEFAULT, plan: Sequence[int] = (7, 1, 0, 2),
                avoid: Sequence[int] = ()) -> Trace:
    """n_new tokens of the float64 oracle under `params` (temperature, top_k, top_p, min_p, repetition_penalty), the draws
    steered through the verify steps of a lookup run with config `lookup`: step s accepts up to plan[s % len(plan)] drafted
    tokens and then leaves the draft.  Tokens in `avoid` (stop ids) are never chosen.  Every precondition is asserted."""
    D, hi, lo = lookup
    pen = params.get("repetition_penalty", 1.0)
    T = params.get("temperature", 1.0)
    tr = Trace()
    hist = list(prompt)
    cache = ref.new()
    row = ref.logits(hist, cache)[-1]

    def state(row64, history):
        P = penalty_factor(history, pen)
        ids, probs, slack = distribution(penalise(row64, history, pen), P=P, **params)
        return ids, probs, slack, P

    def decide(prefer: Sequence[int], history, row64, fresh_first=False):
        """Steers to the first token of `prefer` (then any other, most probable first) that can be steered to and whose
        successor state is clear; returns (token, successor row)."""
        ids, probs, slack, P = state(row64, history)
        assert slack >= 1.0, f"precondition: a filter decision clears its boundary by {slack:.2f} of what is required"
        M = u_margin(P, T)
        rest = [int(t) for t in ids[np.argsort(-probs, kind="stable")] if int(t) not in prefer]
        first = True
        choices = list(prefer) + rest
        if fresh_first:   # a token the run has not emitted yet, so that a stop id can be met for the first time inside a block
            choices.sort(key=lambda t: t in tr.ids)
        for t in choices:
            u = steer(ids, probs, t, M) if t not in avoid else None
            if u is not None:
                nxt = ref.logits([t], probe := list(cache))[-1]
                n_ids, n_probs, n_slack, n_P = state(nxt, history + [t])
                if n_slack >= 1.0 and any(steer(n_ids, n_probs, int(c), u_margin(n_P, T)) is not None for c in n_ids):
                    cache[:] = probe
                    tr.ids.append(t)
                    tr.uniforms.append(u)
                    tr.redraws += 0 if first else 1
                    tr.min_slack = min(tr.min_slack, slack)
                    tr.min_clear = min(tr.min_clear, draw_clearance(probs, u) / M)
                    tr.max_P = max(tr.max_P, P)
                    return t, nxt
                first = False      # (a token that cannot be steered to was never a choice; one with an unclear successor was)
        raise AssertionError("precondition: no token of this state can be steered to with a clear successor")

    seen = lambda: [t for t in dict.fromkeys(reversed(hist))]   # tokens of the history, latest first: picking one makes drafts
    tok, row = decide(seen(), hist, row)
    hist.append(tok)
    step = 0
    while len(tr.ids) < n_new:
        draft = LK.lookup_draft(hist, hi, lo, D)
        want = min(plan[step % len(plan)], len(draft))
        a = 0
        for r in range(len(draft) + 1):
            if len(tr.ids) >= n_new:
                break
            if r < want:
                prefer = [draft[r]] + [t for t in seen() if t != draft[r]]
            else:
                prefer = [t for t in seen() if r >= len(draft) or t != draft[r]]
            tok, row = decide(prefer, hist, row, fresh_first=r == 2 and r >= want)
            hist.append(tok)
            tr.rows.append(r)
            if r < len(draft) and tok == draft[r]:
                a += 1
            else:
                break
        tr.steps.append((len(draft), a))
        step += 1
    assert tr.min_slack >= 1.0 and tr.min_clear >= 1.0
    assert tr.redraws <= MAX_REDRAW_RATE * len(tr.ids), f"{tr.redraws} redraws in {len(tr.ids)} draws: the margins are wrong"
    return tr


def replay(ref, prompt, uniforms, n_new, params, stops=(), context: int = 0):
    """The plain sampled loop of the oracle on given draws (generate()'s order of checks): (ids, draws used, the smallest filter
    slack, the smallest draw clearance in units of U_MARGIN)."""
    pen, T = params.get("repetition_penalty", 1.0), params.get("temperature", 1.0)
    hist, out, used = list(prompt), [], 0
    cache = ref.new()
    row = ref.logits(hist, cache)[-1]
    min_slack = min_clear = float("inf")
    while len(out) < n_new and (not context or len(hist) < context):
        P = penalty_factor(hist, pen)
        ids, probs, slack = distribution(penalise(row, hist, pen), P=P, **params)
        u = float(uniforms[used])
        used += 1
        min_slack, min_clear = min(min_slack, slack), min(min_clear, draw_clearance(probs, u) / u_margin(P, T))
        tok = pick(ids, probs, u)
        if tok in stops:
            break
        hist.append(tok)
        out.append(tok)
        if context and len(hist) >= context:
            break
        row = ref.logits([tok], cache)[-1]
    return out, used, min_slack, min_clear


# ---- blocks for lookup_accept_sampled -----------------------------------------------------------------------------------------------

def accept_block(vocab: int, rows: int, n_draft: int, a_want: int, params: Dict, seed: int):
    """A seeded float32 logits block [rows, vocab], a draft and steered draws for which the float64 oracle accepts exactly
    a_want <= min(n_draft, rows - 1) drafted tokens: (block, draft, uniforms, picks, redraws).  Every draft entry after the
    first rejected one is poison (an id >= vocab that equals no pick): a decision that goes on after the rejection shows.
    Rows whose filters do not clear their boundaries, or that offer fewer than two tokens to steer to, are redrawn from the
    seeded generator (counted); the preconditions hold for what is returned."""
    rng = np.random.default_rng(seed)
    M = u_margin(1.0, params.get("temperature", 1.0))
    last = min(n_draft, rows - 1)
    assert 0 <= a_want <= last
    block = np.empty((rows, vocab), F32)
    draft, uniforms, picks, redraws = [vocab + 7] * n_draft, [], [], 0
    for r in range(rows):
        while True:
            row = (3.5 * rng.standard_normal(vocab)).astype(F32)
            ids, probs, slack = distribution(row, **params)
            steerable = [int(t) for t in ids[np.argsort(-probs, kind="stable")] if steer(ids, probs, int(t), M) is not None]
            if slack >= 1.0 and len(steerable) >= 2:
                break
            redraws += 1
        block[r] = row
        if r > a_want:
            continue                                   # not reached: no draw, the draft stays poison
        picks.append(steerable[0])
        uniforms.append(steer(ids, probs, steerable[0], M))
        if r < n_draft:
            draft[r] = steerable[0] if r < a_want else steerable[1]
    return block, draft, uniforms, picks, redraws


# ---- one teacher-forced block for verify_step_sampled -----------------------------------------------------------------------------

def build_block(ref, prompt: Sequence[int], token: int, n_draft: int, a_want: int, params: Dict, avoid: Sequence[int] = ()):
    """A draft of n_draft tokens after prompt + [token] and steered draws for which the oracle accepts exactly a_want of them:
    (draft, uniforms, picks), or None when some decided row of this prompt does not meet the preconditions (the caller tries
    its next prompt).  Rows 0..a_want are decided: draft[r] is the steered pick for r < a_want -- a token whose successor row
    is clear in its turn, one new to the history when there is a choice (the penalty factor stays small) -- and another token
    the row could have produced at r = a_want; the rows after that continue with their most probable token and are never
    decided."""
    pen, T = params.get("repetition_penalty", 1.0), params.get("temperature", 1.0)
    hist = list(prompt) + [token]
    cache = ref.new()
    ref.logits(list(prompt), cache)
    row = ref.logits([token], cache)[-1]

    def state(row64, history):
        P = penalty_factor(history, pen)
        ids, probs, slack = distribution(penalise(row64, history, pen), P=P, **params)
        M = u_margin(P, T)
        ranked = [int(t) for t in ids[np.argsort(-probs, kind="stable")] if int(t) not in avoid]
        can = [t for t in ranked if steer(ids, probs, t, M) is not None]
        return ids, probs, M, ranked, can, slack >= 1.0 and len(can) >= 2

    draft, uniforms, picks = [], [], []
    for r in range(n_draft + 1):
        ids, probs, M, ranked, can, clear = state(row, hist)
        nxt, nxt_row = None, None
        if r <= a_want:
            if not clear:
                return None
            can.sort(key=lambda t: t in hist)
            if r < a_want:   # the pick is accepted and the next row decided: it has to be clear too
                for c in can:
                    probe = list(cache)
                    succ = ref.logits([c], probe)[-1]
                    if state(succ, hist + [c])[-1]:
                        nxt, nxt_row = c, succ
                        cache[:] = probe
                        break
                if nxt is None:
                    return None
                picks.append(nxt)
            else:
                picks.append(can[0])
                nxt = can[1]
            uniforms.append(steer(ids, probs, picks[-1], M))
        elif ranked:
            nxt = ranked[0]
        else:
            nxt = int(ids[0])
        if r < n_draft:
            draft.append(nxt)
            hist.append(nxt)
            row = nxt_row if nxt_row is not None else ref.logits([nxt], cache)[-1]
    return draft, uniforms, picks


def sharpen(tensors: Dict[str, np.ndarray], factor: float) -> Dict[str, np.ndarray]:
    """The same Llama-layout model with every logit multiplied by `factor` (the final norm's gain): fewer, better separated
    survivors, for filter sets whose preconditions a flat distribution rarely meets."""
    out = dict(tensors)
    out["model.norm.weight"] = (np.asarray(tensors["model.norm.weight"], F32) * F32(factor)).astype(F32)
    return out
