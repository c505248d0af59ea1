"""The device kernels that decide WHICH token comes out, alone, on logits of production vocabularies (kjarni_hip_op_argmax,
kjarni_hip_op_whisper_pick, kjarni_hip_op_logits_processors, kjarni_hip_op_sample_candidates; every entry runs the launcher the
models run).  References are plain NumPy and the oracles; a wrong token is a wrong token, so everything here is exact except
the sampler's sum of exponentials.

  argmax (decoder, lanes and lookup routes): np.flatnonzero(v == v.max())[-1] -- the last of equal maxima, +0.0 == -0.0 --
    with the maxima placed by the launch geometry (same wave, other wave, other workgroup, one grid stride apart).
  Whisper pick (one launch, two launches): oracle/whisper_oracle.py pick_token; the two forms agree.
  logits processors: bit-equal to oracle/llm_oracle.py on an f32 copy (the kernel multiplies and divides with IEEE rounding).
  sampler cut: the header's maximum exact; its sum within 2e-5 relative of the float64 sum (a tenth of the 2e-4 the host's
    top-p scan trusts an out-of-order sum to; worst observed on an MI355X over every call here: 1.39e-7); the candidates exactly
    {i : logits[i] >= floor}; the floor low enough for the filters (float64) and no lower than the kernel's stated margin;
    overflow exactly when the list is too long or no cut exists; the same scratch reused call after call; and the host's
    decision from the device's list equal to the full host sampler bit for bit, and to the oracle up to negligible mass.

The case builders (tests/token_select_cases.py) touch no GPU."""

import numpy as np
import pytest

from kjarni_amd import chat as K
from kjarni_amd import ops
from oracle import chat_oracle as co
from oracle import whisper_oracle as W
from oracle.llm_oracle import apply_no_repeat_ngram, apply_repetition_penalty
from tests import token_select_cases as T
from tests.parity_report import report

pytestmark = pytest.mark.gpu

VOCABS = (1, 63, 257, 720, 2048, 2049, 50257, 128256, 151936, 600000)   # 600 000: launch_argmax's 256 workgroups take a second trip
SUM_TOL = 2e-5
PAD = np.float32(3e38)    # columns vocab .. ld of a row: larger than every logit, and not part of the vocabulary


# ------------------------------------------------------------------------------------------------------------------ argmax
def _rows(vocab):
    cases = T.argmax_cases(vocab)
    return [n for n, _, _ in cases], np.stack([v for _, v, _ in cases]), np.array([T.last_max(v) for _, v, _ in cases], np.int32)


def _wrong(names, got, want):
    return [(n, int(g), int(w)) for n, g, w in zip(names, got, want) if g != w]


@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_decoder_route(vocab):
    names, rows, want = _rows(vocab)
    got = ops.argmax(rows[:, None, :], route=ops.ARGMAX_DECODER)[:, 0]
    assert not _wrong(names, got, want), f"vocab {vocab}: (case, device, last maximum) {_wrong(names, got, want)}"


def _groups_of_8(rows, want, ld):
    """The cases as calls of 8 rows [calls, 8, ld] (the last call repeats the first cases), padding columns at PAD."""
    n = rows.shape[0]
    idx = np.arange(-(-n // 8) * 8) % n
    out = np.full((idx.size, ld), PAD, np.float32)
    out[:, :rows.shape[1]] = rows[idx]
    return idx, out.reshape(-1, 8, ld), want[idx].reshape(-1, 8)


@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_lanes_route(vocab):
    """8 rows, a mixed live mask and its complement (every case is picked once), ld > vocab: a frozen lane yields nothing and
    the entry checks that its token and history came back untouched and the accumulators zeroed."""
    names, rows, want = _rows(vocab)
    idx, calls, want8 = _groups_of_8(rows, want, vocab + 5)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.int32)
    for live in (mask, 1 - mask):
        got = ops.argmax(calls, vocab=vocab, route=ops.ARGMAX_LANES, live=live)
        assert (got[:, live == 0] == -1).all()
        on = np.flatnonzero(live)
        bad = _wrong([names[i] for i in idx.reshape(-1, 8)[:, on].ravel()], got[:, on].ravel(), want8[:, on].ravel())
        assert not bad, f"vocab {vocab}, live {live.tolist()}: (case, device, last maximum) {bad}"
    if vocab == 720:   # fewer lanes than 8, all live, ld == vocab
        got = ops.argmax(rows[None, :3, :], route=ops.ARGMAX_LANES, live=[1, 1, 1])
        assert got[0].tolist() == want[:3].tolist()


@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_lookup_route(vocab):
    """The verify pick on 8 rows: a draft equal to the rows' own last maxima is accepted whole (so every row's pick is seen);
    with one drafted id replaced, the accepted count is the longest matching prefix and the picks stop after the correction."""
    names, rows, want = _rows(vocab)
    idx, calls, want8 = _groups_of_8(rows, want, vocab + 3)
    case_names = np.array(names)[idx].reshape(-1, 8)
    draft = want8[:, :7].astype(np.uint32)
    picks, acc = ops.argmax(calls, vocab=vocab, route=ops.ARGMAX_LOOKUP, draft=draft)
    bad = _wrong(case_names.ravel(), picks.ravel(), want8.ravel())
    assert not bad, f"vocab {vocab}: (case, device, last maximum) {bad}"
    assert acc.tolist() == [7] * len(calls)
    for n_draft, shift in ((7, 0), (7, 3), (3, 1), (1, 0), (0, 0)):
        d = want8[:, :n_draft].astype(np.uint32)
        for c in range(len(calls)):
            if n_draft:
                j = (c + shift) % n_draft
                d[c, j] = (d[c, j] + 1) % max(vocab, 2)            # another id: rows j + 1 .. are rejected
        picks, acc = ops.argmax(calls[:, :n_draft + 1 + (n_draft == 3)], vocab=vocab, route=ops.ARGMAX_LOOKUP,
                                draft=d if n_draft else None)      # (n_draft 3 runs with one pad row, as a short draft does)
        for c in range(len(calls)):
            a = T.accepted_prefix(d[c], want8[c])
            assert acc[c] == a and a < max(n_draft, 1), (vocab, n_draft, c)
            assert picks[c, :a + 1].tolist() == want8[c, :a + 1].tolist(), (vocab, n_draft, c, case_names[c].tolist())
            assert (picks[c, a + 1:] == -1).all()


# ------------------------------------------------------------------------------------------------------------ whisper pick
@pytest.mark.parametrize("vocab", [51865, 51866])
@pytest.mark.parametrize("timestamps", [False, True])
def test_whisper_pick_both_forms(vocab, timestamps):
    fs, eos, tb = W.FIRST_SPECIAL_TOKEN, W.EOT_TOKEN, W.TIMESTAMP_BEGIN
    cases = T.whisper_cases(vocab, fs, eos, tb)
    names = [n for n, _ in cases]
    rows = np.stack([v for _, v in cases])
    want = np.array([W.WhisperOracle.pick_token(v, timestamps, eos) for v in rows], np.int32)
    allowed = (want < fs) | (want == eos) | (timestamps & (want >= tb))
    assert allowed.all() and len(set(want.tolist())) > 8              # (the cases do not all collapse onto one id)
    n4 = -(-len(cases) // 4) * 4
    idx4 = np.arange(n4) % len(cases)
    got = {}
    for two_launch in (False, True):
        one = ops.whisper_pick(rows[:, None, :], fs, eos, tb, timestamps, two_launch)[:, 0]
        four = ops.whisper_pick(rows[idx4].reshape(-1, 4, vocab), fs, eos, tb, timestamps, two_launch).ravel()
        bad = _wrong(names, one, want) + _wrong([names[i] for i in idx4], four, want[idx4])
        assert not bad, f"vocab {vocab}, timestamps {timestamps}, two launches {two_launch}: (case, device, pick_token) {bad}"
        got[two_launch] = (one, four)
    assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])


# ------------------------------------------------------------------------------------------------------ logits processors
@pytest.mark.parametrize("vocab", [50257, 151936])
@pytest.mark.parametrize("ngram", [0, 1, 2, 3, 5])
def test_logits_processors_bit_exact(vocab, ngram):
    banned_some = False
    for length in sorted({0, 1, ngram - 1, ngram, 300, 2000} - {-1}):
        hist = T.processor_history(vocab, length, ngram, seed=100 * length + ngram)
        assert len(hist) == length
        if length >= 300:
            assert max(np.bincount(np.array(hist))) >= 24 and max(hist) >= vocab     # a token recurs dozens of times; one id is no token
        logits = T.processor_logits(vocab, hist)
        for penalty in (1.3, 0.8, 2.0):
            want = logits.copy()
            with np.errstate(over="ignore"):     # (a token that recurs hundreds of times is divided by 0.8 up to +inf: on both sides)
                apply_repetition_penalty(want, hist, penalty)
            if ngram > 0:
                before = np.isneginf(want).sum()
                apply_no_repeat_ngram(want, hist, ngram)
                banned_some |= bool(np.isneginf(want).sum() > before)
            for n_bulk in sorted({0, length // 2, length}):
                got = ops.logits_processors(logits, hist, n_bulk, penalty, ngram)
                diff = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
                assert np.array_equal(got, want), (vocab, ngram, length, penalty, n_bulk, diff[:5], got[diff[:5]], want[diff[:5]])
    assert banned_some == (ngram > 0)


# ------------------------------------------------------------------------------------------------------------ sampler cut
def _filters(p):
    return {k: v for k, v in p.items() if k != "temperature"}


def _check_call(name, params, h, capacity):
    """Items 1-6 of the cut's contract for one call's header + candidates; returns the relative error of the sum."""
    logits = T.sampler_logits(name)
    V = logits.size
    f = _filters(params)
    tag = (name, params, capacity)
    assert h["mx"] == logits.max(), tag                                                    # 1
    want_sum = T.exp_sum(name)
    err = abs(float(h["sum"]) - want_sum) / want_sum
    print(f"{name} {f} capacity {capacity}: sum rel err {err:.3e} count {h['count']} overflow {h['overflow']} "
          f"mx - floor {float(h['mx']) - float(h['floor']):.4f}")
    assert err <= SUM_TOL, (tag, err)                                                      # 2
    no_cut = T.no_cut_exists(V, **f) or not np.isfinite(logits.max())
    members = np.flatnonzero(logits >= h["floor"])
    assert h["count"] == members.size, (tag, h["count"], members.size)                     # 3 / 4: the true size, overflowing or not
    assert h["overflow"] == int(members.size > capacity or no_cut), (tag, h["overflow"], members.size)   # 4
    if no_cut:               # nothing was appended: the host takes the logits
        assert h["floor"] == -np.inf, tag
        return err
    ids = h["ids"].astype(np.int64)
    assert ids.size == min(members.size, capacity)
    assert np.unique(ids).size == ids.size and (ids < V).all(), tag                        # no duplicates
    assert np.array_equal(h["logits"], logits[ids]), tag                                   # each carries its own logit
    if not h["overflow"]:
        assert np.array_equal(np.sort(ids), members), tag                                  # 3: exactly the set
    else:
        assert np.isin(ids, members).all(), tag
    reach = float(h["mx"]) - float(h["floor"])
    need = T.needed_distance(name, **f)
    assert reach >= need, (tag, reach, need)                                               # 5
    tight = T.needed_distance(name, p_inflate=1.001, **f)
    assert reach <= tight + 0.5, (tag, reach, tight)                                       # 6
    return err


def _decide(name, params, h):
    """The host's decision from the device's list: None when declined or overflowed, else probs -- which must be the full host
    sampler's bit for bit, and the oracle's up to mass below 1e-5."""
    if h["overflow"]:
        return None
    logits = T.sampler_logits(name)
    got = K.sampling_distribution_from_candidates(h["ids"], h["logits"], h["mx"], h["floor"], h["sum"], logits.size, **params)
    if got is None:
        return None
    assert np.array_equal(got, K.sampling_distribution(logits, **params)), (name, params)
    want = co.sampling_distribution(logits, params.get("temperature", 1.0), params.get("top_k"), params.get("top_p"), params.get("min_p"))
    diff = np.flatnonzero((want > 0) != (got > 0))
    assert np.maximum(want, got)[diff].sum() < 1e-5, (name, params, diff[:5])
    return got


@pytest.mark.parametrize("params", T.SAMPLER_PARAMS, ids=lambda p: "-".join(f"{k}={v}" for k, v in p.items()) or "nothing-set")
def test_sampler_cut(params):
    """Every logit set, one after another on one scratch (as consecutive tokens are), at the models' capacity."""
    heads = ops.sample_candidates([T.sampler_logits(n) for n in T.SAMPLER_SETS], capacity=4096, **params)
    worst = 0.0
    decided = 0
    for name, h in zip(T.SAMPLER_SETS, heads):
        worst = max(worst, _check_call(name, params, h, 4096))
        decided += _decide(name, params, h) is not None
    report("sampler cut: relative error of the device sum", worst, SUM_TOL)
    if not any(k in params for k in ("top_k", "top_p", "min_p")):
        assert decided == 0      # temperature only needs the whole vocabulary


def test_sampler_cut_small_capacity_overflows_into_nothing():
    """The same call at capacity 4096 and at 64: the second overflows, reports the true count and stays inside its 64 slots
    (the entry checks the guard band behind them)."""
    name, params = "zipf-128256-1.3", dict(top_k=40, top_p=0.9, min_p=0.05)
    big, = ops.sample_candidates([T.sampler_logits(name)], capacity=4096, **params)
    small, = ops.sample_candidates([T.sampler_logits(name)], capacity=64, **params)
    _check_call(name, params, big, 4096)
    _check_call(name, params, small, 64)
    assert big["overflow"] == 0 and small["overflow"] == 1 and 64 < small["count"] == big["count"]
    assert (small["mx"], small["sum"], small["floor"]) == (big["mx"], big["sum"], big["floor"])


@pytest.mark.parametrize("params", [dict(top_k=40, top_p=0.9, min_p=0.05), dict(top_p=0.9, min_p=0.05), dict(top_k=3000)],
                         ids=["k40-p0.9-minp0.05", "p0.9-minp0.05", "k3000"])
def test_sampler_scratch_reuse(params):
    """Four tokens on one scratch and header: a peaked row, a flat one that overflows, a vocabulary of 257 (the other 61
    workgroups' partial slots hold the previous rows' values unless rewritten) and the first row again, which must give the
    first call's maximum and sum bit for bit."""
    names = ["zipf-128256-1.3", "flat", "small-257", "zipf-128256-1.3"]
    heads = ops.sample_candidates([T.sampler_logits(n) for n in names], capacity=4096, **params)
    for name, h in zip(names, heads):
        _check_call(name, params, h, 4096)
        _decide(name, params, h)
    assert heads[1]["overflow"] == 1 and heads[0]["overflow"] == 0
    first, again = heads[0], heads[3]
    assert first["mx"].tobytes() == again["mx"].tobytes() and first["sum"].tobytes() == again["sum"].tobytes()
    assert first["floor"] == again["floor"] and first["count"] == again["count"]
    assert np.array_equal(np.sort(first["ids"]), np.sort(again["ids"]))


def test_sampler_declines_rarely():
    """Declining is always allowed to the host, so it could hide a failure: of the 21 everyday combinations at most 2 may be
    declined or overflow.  (The host sampler fed the histogram rule's tau and a double-precision sum declines exactly one:
    vocabulary 128 256 with top-p 0.9 + min-p 0.05, a crossing within rounding; its candidate counts run from 1 to 3 506.)"""
    undecided = []
    counts = []
    for params in T.DECIDING_PARAMS:
        heads = ops.sample_candidates([T.sampler_logits(n) for n in T.DECIDING_SETS], capacity=4096, **_filters(params))
        for name, h in zip(T.DECIDING_SETS, heads):
            _check_call(name, params, h, 4096)
            counts.append(h["count"])
            if _decide(name, params, h) is None:
                undecided.append((name, params, h["count"], h["overflow"]))
    print("undecided:", undecided, "candidate counts", min(counts), "..", max(counts))
    assert len(counts) == 21 and len(undecided) <= 2, undecided
    assert 1 <= min(counts) and max(counts) <= 4096
