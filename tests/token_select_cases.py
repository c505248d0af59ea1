"""Case generators and float64 references for tests/test_gpu_token_select.py.  Nothing here touches a GPU, so every case and
every expected value can be evaluated anywhere.

Launch geometry the cases are placed by (llm_kernels.hip / whisper_kernels.hip): the argmax kernels run 256-thread workgroups
(4 waves of 64), ceil(vocab / 2048) of them, capped at 256 (launch_argmax) or 64 (launch_lane_pick, launch_lookup_pick); element
i belongs to workgroup (i // 256) % blocks, thread i % 256, and a thread revisits i + blocks * 256.  Whisper's two-launch pick runs
48 workgroups of 256, its one-launch form one workgroup of 1024."""
import functools
import math

import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def last_max(v: np.ndarray) -> int:
    """Iterator::max_by with partial_cmp: the LAST of equal maxima (+0.0 == -0.0)."""
    return int(np.flatnonzero(v == v.max())[-1])


# ---------------------------------------------------------------------------------------------------------------- argmax
def argmax_blocks(vocab: int):
    """(workgroups of launch_argmax, workgroups of the lanes / lookup picks)."""
    b = (vocab + 2047) // 2048
    return min(b, 256), min(b, 64)


def argmax_cases(vocab: int):
    """[(name, row f32 [vocab], intended answer)]; only the cases that exist at this vocabulary."""
    rng = np.random.default_rng(1000 + vocab)
    V = vocab
    cases = []

    def base():
        return (rng.standard_normal(V) * 2.0).astype(F32)

    def planted(name, idx):
        v = base()
        top = F32(v.max() + F32(1.0))
        for i in idx:
            v[i] = top
        cases.append((name, v, max(idx)))

    for i in sorted({0, V - 1, 2047, 2048, int(rng.integers(0, V))}):
        if i < V:
            planted(f"unique@{i}", [i])
    if V >= 2:
        a = 64 * int(rng.integers(0, (V - 2) // 64 + 1))
        planted("tie-same-wave", [a, a + 1])
    if V > 64:
        a = 256 * int(rng.integers(0, (V - 65) // 256 + 1))
        planted("tie-other-wave", [a + 3, a + 64 + 3] if a + 67 < V else [a, a + 64])
    strides = sorted({b * 256 for b in argmax_blocks(V)})
    if max(argmax_blocks(V)) > 1:          # more than one workgroup: neighbours in the grid, and the first and the last
        a = int(rng.integers(0, V - 256))
        planted("tie-other-workgroup", [a, a + 256])
        planted("tie-first-last-workgroup", [5, V - 1])
    for s in strides:                      # one grid stride apart: the same thread meets both
        if V > s:
            a = int(rng.integers(0, V - s))
            planted(f"tie-stride-{s}", [a, a + s])
            if V > 2 * s:
                a = int(rng.integers(0, V - 2 * s))
                planted(f"tie-two-strides-{s}", [a, a + 2 * s])
    cases.append(("all-equal", np.full(V, 1.5, F32), V - 1))
    cases.append(("all-neg-inf", np.full(V, NEG_INF, F32), V - 1))
    if V >= 2:
        lo, hi = sorted(int(x) for x in rng.choice(V, 2, replace=False))
        for name, first, second in (("pos-zero-then-neg-zero", 0.0, -0.0), ("neg-zero-then-pos-zero", -0.0, 0.0)):
            v = (-np.abs(base()) - F32(0.5)).astype(F32)
            v[lo], v[hi] = F32(first), F32(second)
            cases.append((name, v, hi))
        v = (-np.abs(base()) - F32(0.5)).astype(F32)   # the two zeros in one wave, adjacent lanes
        a = 64 * int(rng.integers(0, (V - 2) // 64 + 1))
        v[a], v[a + 1] = F32(0.0), F32(-0.0)
        cases.append(("zeros-same-wave", v, a + 1))
    v = (-np.abs(base()) - F32(3.0)).astype(F32)
    i = int(rng.integers(0, V))
    v[i] = F32(-2.5)
    cases.append(("negative-maximum", v, i))
    v = (-np.abs(base()) - F32(0.5)).astype(F32)
    i = int(rng.integers(0, V))
    v[i] = F32(1e-40)
    if V >= 2:
        v[(i + V // 2) % V if (i + V // 2) % V != i else (i + 1) % V] = F32(5e-41)  # a smaller subnormal must lose
    cases.append(("subnormal-maximum", v, i))
    for name, v, want in cases:
        assert v.dtype == F32 and v.shape == (V,) and last_max(v) == want, (vocab, name)
    return cases


def accepted_prefix(draft, picks) -> int:
    """The verify rule: the longest prefix of the draft that equals the rows' own picks."""
    a = 0
    while a < len(draft) and int(draft[a]) == int(picks[a]):
        a += 1
    return a


# ---------------------------------------------------------------------------------------------------------- whisper pick
def whisper_cases(vocab: int, first_special: int, eos: int, timestamp_begin: int):
    """[(name, row f32 [vocab])]: expected values come from the oracle's pick_token, for timestamps off and on."""
    rng = np.random.default_rng(2000 + vocab)
    V = vocab
    cases = []

    def base():
        return (rng.standard_normal(V) * 2.0).astype(F32)

    def planted(name, idx, v=None):
        v = base() if v is None else v
        top = F32(np.abs(v[np.isfinite(v)]).max() + F32(1.0))
        for i in idx:
            v[i] = top
        cases.append((name, v))

    band = int(rng.integers(first_special + 1, timestamp_begin))      # suppressed whatever the timestamps flag says
    text = int(rng.integers(0, first_special))
    stamp = int(rng.integers(timestamp_begin, V))
    planted("text", [text])
    planted("timestamp", [stamp])
    planted("maximum-suppressed", [band])
    planted("maximum-eos", [eos])
    planted("maximum-last-id", [V - 1])
    planted("tie-allowed-suppressed", [text, band])
    planted("tie-suppressed-first", [band, V - 1])
    planted("tie-eos-timestamp", [eos, stamp])
    planted("tie-text-eos", [text, eos])
    planted("tie-other-workgroup", [100, 100 + 256 * 5])
    planted("tie-other-wave", [4096 + 7, 4096 + 64 + 7])
    planted("tie-two-launch-stride", [300, 300 + 48 * 256])
    planted("tie-one-launch-stride", [301, 301 + 1024])
    v = base()
    v[:first_special] = NEG_INF
    v[eos] = NEG_INF
    v[timestamp_begin:] = NEG_INF
    cases.append(("every-allowed-neg-inf", v))
    v = base()
    v[:first_special] = NEG_INF
    v[eos] = NEG_INF                       # timestamps off: nothing finite may be produced; on: a timestamp wins
    cases.append(("text-and-eos-neg-inf", v))
    lo, hi = sorted(int(x) for x in rng.choice(first_special, 2, replace=False))
    for name, first, second in (("pos-zero-then-neg-zero", 0.0, -0.0), ("neg-zero-then-pos-zero", -0.0, 0.0)):
        v = (-np.abs(base()) - F32(0.5)).astype(F32)
        v[lo], v[hi] = F32(first), F32(second)
        cases.append((name, v))
    v = (-np.abs(base()) - F32(0.5)).astype(F32)   # a zero in the suppressed band above both: still the later allowed zero
    v[lo], v[hi], v[band] = F32(-0.0), F32(0.0), F32(0.0)
    cases.append(("zeros-and-suppressed-zero", v))
    return cases


# ------------------------------------------------------------------------------------------------------ logits processors
OUT_OF_VOCAB = 7      # added to the vocabulary size: an id both sides ignore


def processor_logits(vocab: int, history):
    """Positives, negatives, exact zeros and a few -inf, some of each at tokens of the history."""
    rng = np.random.default_rng(3000 + vocab)
    v = (rng.standard_normal(vocab) * 3.0).astype(F32)
    v[rng.integers(0, vocab, 200)] = F32(0.0)
    v[rng.integers(0, vocab, 20)] = NEG_INF
    seen = [t for t in dict.fromkeys(history) if t < vocab]
    for j, t in enumerate(seen[:12]):
        v[t] = (F32(0.0), NEG_INF, F32(2.75), F32(-1.25))[j % 4]
    return v


def processor_history(vocab: int, length: int, ngram: int, seed: int):
    """`length` ids from a Zipf law over a permutation of the vocabulary (the frequent ones recur dozens of times in a long
    history).  Long histories end in a copy of an earlier window, so that an n-gram ban has matches whatever n is; one of the
    tokens such a match would ban is >= vocab."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(vocab)
    h = perm[(rng.zipf(1.3, length) - 1) % vocab].astype(np.int64)
    k = max(ngram - 1, 1)
    if length >= 4 * k + 8:
        src = int(rng.integers(0, length // 2 - k))
        h[length - k:] = h[src:src + k]                   # the tail repeats h[src : src + k]: h[src + k] is banned
        src2 = int(rng.integers(length // 2, length - 2 * k - 2))
        h[src2:src2 + k] = h[length - k:]
        h[src2 + k] = vocab + OUT_OF_VOCAB                # a second match whose continuation is not a token
    elif length >= 2:
        h[int(rng.integers(0, length))] = vocab + OUT_OF_VOCAB
    return [int(t) for t in h]


# ------------------------------------------------------------------------------------------------------------ sampler cut
def zipf_logits(V: int, a: float):
    rng = np.random.default_rng(V)
    ranks = rng.permutation(V) + 1
    return (-a * np.log(ranks) + 0.3 * rng.standard_normal(V)).astype(F32)


@functools.lru_cache(maxsize=None)
def sampler_logits(name: str):
    rng = np.random.default_rng(4000 + sum(map(ord, name)))
    if name.startswith("zipf-"):
        _, V, a = name.split("-")
        v = zipf_logits(int(V), float(a))
    elif name == "flat":
        v = (0.05 * rng.standard_normal(128256)).astype(F32)
    elif name == "lone":
        v = np.full(128256, -30.0, F32)
        v[-1] = F32(5.0)
    elif name == "banned":
        v = zipf_logits(128256, 1.3).copy()
        v[rng.choice(128256, 1000, replace=False)] = NEG_INF
    elif name == "ties":
        v = np.round(2.0 * rng.standard_normal(32000)).astype(F32)
    elif name.startswith("small-"):
        v = (2.5 * rng.standard_normal(int(name.split("-")[1]))).astype(F32)
    else:
        raise KeyError(name)
    v.setflags(write=False)
    return v


SAMPLER_SETS = ("zipf-128256-1.3", "zipf-50257-1.5", "zipf-32000-2.0", "zipf-151936-1.1", "flat", "lone", "banned", "ties", "small-720",
                "small-257")
SAMPLER_PARAMS = (dict(top_k=40, top_p=0.9, min_p=0.05), dict(top_p=0.9, min_p=0.05), dict(top_k=5), dict(top_k=1), dict(top_p=0.5),
                  dict(min_p=0.2), dict(top_k=3000), dict(top_k=5000), dict(top_p=0.999), dict(top_p=1.0), dict(min_p=0.0), dict())
# the combinations of which at most two may be declined or overflow (temperature as a chat mode would set it)
DECIDING_SETS = ("zipf-128256-1.3", "zipf-50257-1.5", "zipf-32000-2.0")
DECIDING_PARAMS = (dict(top_k=40, top_p=0.9, min_p=0.05, temperature=0.7), dict(top_p=0.9, min_p=0.05, temperature=0.6), dict(top_k=5),
                   dict(top_k=1), dict(top_p=0.5), dict(min_p=0.2, temperature=1.3), dict(top_k=3000))


@functools.lru_cache(maxsize=None)
def _sorted_mass(name: str):
    """The set's values in descending order, and the running sum of exp(v - max), in float64."""
    v = np.sort(sampler_logits(name).astype(np.float64))[::-1]
    cum = np.cumsum(np.exp(v - v[0]))
    return v, cum


def exp_sum(name: str) -> float:
    """float64 sum of exp(v - max) over the set."""
    v = sampler_logits(name).astype(np.float64)
    return float(math.fsum(np.exp(v - v.max())))


def no_cut_exists(vocab: int, top_k=None, top_p=None, min_p=None) -> bool:
    """The parameter sets for which no finite floor decides the filters: top-p 1.0 keeps the whole mass, min-p 0 alone keeps
    everything."""
    k_on = top_k is not None and top_k < vocab
    p_on = top_p is not None and top_p < 1.0
    return (top_p is not None and top_p >= 1.0) or (min_p is not None and min_p <= 0.0 and not k_on and not p_on)


def needed_distance(name: str, top_k=None, top_p=None, min_p=None, p_inflate: float = 1.0) -> float:
    """How far below the maximum the filters reach, in float64: the k-th largest value (top-k < vocab), the value at which
    the descending cumulative mass first exceeds top_p * p_inflate * total, and ln(1 / min_p) when min-p is the only filter."""
    v, cum = _sorted_mass(name)
    V = v.size
    d = 0.0
    k_on = top_k is not None and top_k < V
    if k_on:
        d = max(d, v[0] - v[max(top_k, 1) - 1])
    if top_p is not None:
        j = int(np.searchsorted(cum, top_p * p_inflate * cum[-1], side="right"))   # first j with cum[j] > target
        d = max(d, v[0] - v[j] if j < V else math.inf)
    if min_p is not None and not k_on and top_p is None:
        d = max(d, math.log(1.0 / min_p) if min_p > 0.0 else math.inf)
    return float(d)
