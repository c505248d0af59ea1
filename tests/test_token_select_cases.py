"""The references of tests/test_gpu_token_select.py, held to a NumPy restatement of the sampler's histogram rule and to the
host sampler, without a GPU: a reference that is wrong would otherwise only show as a device failure."""
import math

import numpy as np

from kjarni_amd import chat as K
from tests import token_select_cases as T


def _histogram_tau(v, top_k=None, top_p=None, min_p=None):
    """sample_compact_kernel's cut (llm_kernels.hip) in float64: bins of 1/8 below the maximum, the first bin at which the
    running count holds top_k tokens and the running mass exceeds top_p * 1.001 of the total, two bins of margin; ln(1 / min_p)
    + 0.25 when min-p filters the whole vocabulary."""
    m = v.max()
    d = (m - v) * np.float32(8.0)
    b = np.where(d < 512, d, 512).astype(np.int64)
    e = np.exp(v.astype(np.float64) - float(m))
    count = np.cumsum(np.bincount(b, minlength=513)[:512])
    mass = np.cumsum(np.bincount(b, weights=e, minlength=513)[:512])
    k_on = top_k is not None and top_k < v.size
    need_mass = top_p * e.sum() * 1.001 if top_p is not None else 0.0
    ok = np.flatnonzero((count >= (top_k if k_on else 1)) & (mass > need_mass))
    tau = (ok[0] + 2) / 8 if ok.size else math.inf
    if min_p is not None and not k_on and not (top_p is not None and top_p < 1.0):
        tau = max(tau, -math.log(min_p) + 0.25) if min_p > 0 else math.inf
    return tau


def test_argmax_and_whisper_cases_build_at_every_vocabulary():
    for vocab in (1, 63, 257, 720, 2048, 2049, 50257):
        cases = T.argmax_cases(vocab)            # (asserts that the rule gives each case's intended answer)
        names = [n for n, _, _ in cases]
        assert len(set(names)) == len(names) and ("tie-same-wave" in names) == (vocab >= 2)
    names = [n for n, _, _ in T.argmax_cases(600000)]
    assert "tie-stride-65536" in names and "tie-stride-16384" in names     # the 256- and the 64-workgroup caps
    assert len(T.whisper_cases(51865, 50257, 50257, 50364)) >= 16


def test_needed_distance_brackets_the_histogram_rule():
    """Completeness and tightness as the GPU test asserts them hold for the rule itself, with the margin the kernel states:
    tau exceeds the inflated need by 0.125 .. 0.25."""
    lo, hi = math.inf, -math.inf
    for name in T.SAMPLER_SETS:
        v = T.sampler_logits(name)
        for p in T.SAMPLER_PARAMS:
            tau = _histogram_tau(v, **p)
            assert T.no_cut_exists(v.size, **p) == (not math.isfinite(tau)), (name, p)
            if not math.isfinite(tau):
                continue
            tight = T.needed_distance(name, p_inflate=1.001, **p)
            assert T.needed_distance(name, **p) <= tau <= tight + 0.5, (name, p, tau, tight)
            lo, hi = min(lo, tau - tight), max(hi, tau - tight)
    assert 0.125 <= lo and hi <= 0.25, (lo, hi)


def test_host_sampler_declines_at_most_one_of_the_everyday_combinations():
    declined, counts = [], []
    for name in T.DECIDING_SETS:
        v = T.sampler_logits(name)
        for p in T.DECIDING_PARAMS:
            tau = _histogram_tau(v, **{k: x for k, x in p.items() if k != "temperature"})
            got, n = K.sampling_distribution_candidates(v, tau, **p)
            counts.append(n)
            if got is None:
                declined.append((name, p))
    # (the one crossing that lies within the rounding of the sum; whether it is declined hangs on the last bits of that sum)
    assert all(d == ("zipf-128256-1.3", dict(top_p=0.9, min_p=0.05, temperature=0.6)) for d in declined), declined
    assert (min(counts), max(counts)) == (1, 3506)
