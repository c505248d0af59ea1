"""Generation log-probabilities on the GPU (kjarni_hip_op_token_logprobs, kjarni_hip_decoder_generate_logprobs,
kjarni_hip_decoder_generate_wide_logprobs, Generator / Chat set_logprobs).

The kernel pair alone against float64 and against the pick kernels; then every loop: the ids first (bit-equal to the entry without
log-probabilities, same options and draws), then the records against the float64 references fed the emitted ids, so that
row i is the raw logits row token i was decided from -- whatever mask, processor or sampler decided it.

Bars.  The op works on given logits: logprob, lse and the top-k logprobs get 2 * 1e-4 * max(1, max |logits|), the bar of the
score-head op tests (tests/test_gpu_score.py), and the top-k ids are exact (the inputs are the same bits on both sides, so the
tie rule decides).  The loops: 2 * 1e-4 * max(1, max |ref logits|) (score()'s bar, for score()'s reason: lse is 1-Lipschitz in
the sup norm); slot j's logprob is held to the j-th largest float64 log-probability whichever id the device chose; ids are
compared only in slots whose float64 logit is at least lanes_cases.GAP away from both neighbours of the sorted list; at most
2 % of a case's slots may be left out, none in a case of fewer than 50.  The seeds below were chosen with the references alone
(tools/gen_logprobs_seed_search.py); every test asserts the margins again."""
import os
import shutil

import numpy as np
import pytest

from tests import constraint_cases as CC
from tests import gen_logprobs_ref64 as R
from tests import gpt2_fixture as G
from tests import grammar_cases as GC
from tests import lanes_cases as LC
from tests import sampled_lookup_cases as SC
from tests import synth
from tests import wide_cases as WC

pytestmark = pytest.mark.gpu
TOL = 1e-4
NAN = np.float32(np.nan)
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. the op alone -----------------------------------------------------------------------------------------------------------------

def _op_rows(V, rows, seed, first_kind=0):
    """rows x V float32 logits: seeded normal rows, with the hand-made rows of the issue in fixed places (row r is of kind
    (r + first_kind) % 8: a one-row shape sees every kind through first_kind)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, V)) * 3.0).astype(np.float32)
    L = R.slab_len(rows, V)
    for r in range(rows):
        kind = (r + first_kind) % 8
        if kind == 1 and V > 8:                          # equal maxima in two slabs, at both ends of a slab, first and last element
            for c in {0, min(L - 1, V - 1), min(L, V - 1), V - 1, V // 2}:
                x[r, c] = 21.5
        elif kind == 2:                                  # an all-equal row
            x[r, :] = -3.25
        elif kind == 3:                                  # -inf entries, the two zeros among the best
            x[r, ::3] = -np.inf
            x[r, 1], x[r, V - 2] = 0.0, -0.0
            x[r, np.isfinite(x[r]) & (x[r] > 0)] *= -1.0
        elif kind == 4:                                  # +-60 and one +88: exp() of the raw values overflows float32
            x[r, ::2], x[r, 1::2] = 60.0, -60.0
            x[r, V // 3] = 88.0
        elif kind == 5:                                  # every other logit underflows: lse is the maximum exactly
            x[r, :] = -200.0
            x[r, V - 1 - (V > 1)] = 7.0
    return x


def _op_tokens(V, rows, x):
    """Element 0, vocab - 1, the tail behind the last whole 16-byte load, a slab's first column, the row's arg-max; some -1."""
    L = R.slab_len(rows, V)
    special = [0, V - 1, max(V - 1 - (V % 4 > 1), 0), min(L, V - 1), None, -1, V // 2]
    tk = np.empty(rows, np.int32)
    for r in range(rows):
        s = special[(r + rows) % 7]
        tk[r] = int(R.topk_ids(x[r], 1)[0]) if s is None else s
    if rows == 1:
        tk[0] = V - 1
    return tk


def _argmax_rows(x, V):
    """kjarni_hip_op_argmax on the same rows, eight at a time (lanes route; one row: the decoder's pick)."""
    from kjarni_amd import ops
    rows = x.shape[0]
    if rows == 1:
        return ops.argmax(x[None, :, :], V)[0]
    out = []
    for r in range(0, rows, 8):
        blk = x[r:r + 8]
        out.append(ops.argmax(blk[None, :, :], V, route=ops.ARGMAX_LANES, live=np.ones(blk.shape[0], np.int32))[0])
    return np.concatenate(out)


def _check_op(x, V, tk, k, what, recs=None):
    """recs (optional): a dict the float64 records of the rows are kept in at top_k 8, for the next top_k of the same rows."""
    from kjarni_amd import ops
    rows, ld = x.shape
    calls = np.stack([x, x])                              # the same rows twice: call 0 reads the row, call 1 takes and reads the copy
    toks = np.stack([tk, tk])
    init = (np.full((2, rows), 7.5, np.float32), np.full((2, rows, k), 1234567, np.uint32), np.full((2, rows, k), 7.5, np.float32),
            np.full((2, rows), 7.5, np.float32))
    got = ops.token_logprobs(calls, toks, k, vocab=V, out=init)
    again = ops.token_logprobs(calls, toks, k, vocab=V, out=init)       # the same call, run twice: the same bits
    assert got["slabs"] == R.slabs(rows, V), what
    for name in ("logprob", "lse", "topk_ids", "topk_logprob"):
        assert _same_bits(got[name], again[name]), f"{what}: {name}: the same call gave other bits"
    for name in ("logprob", "lse", "topk_ids", "topk_logprob"):
        assert _same_bits(got[name][0], got[name][1]), f"{what}: {name}: the two calls differ"
    skip = tk < 0
    assert (got["logprob"][0][skip] == 7.5).all() and (got["lse"][0][skip] == 7.5).all(), f"{what}: a skipped row was written"
    if k:
        assert (got["topk_ids"][0][skip] == 1234567).all() and (got["topk_logprob"][0][skip] == 7.5).all(), f"{what}: a skipped row"
    xv = x[:, :V]
    bar = 2.0 * TOL * max(1.0, float(np.abs(xv[np.isfinite(xv)]).max()))
    live = np.flatnonzero(~skip)
    for r in live:
        if recs is None:
            rec = R.record(xv[r], int(tk[r]), k)
        else:
            if r not in recs:
                recs[r] = R.record(xv[r], int(tk[r]), min(8, V))
            rec = dict(recs[r], topk_ids=recs[r]["topk_ids"][:k], topk_logprob=recs[r]["topk_logprob"][:k])
        assert abs(float(got["lse"][0][r]) - rec["lse"]) <= bar, f"{what}: row {r} lse {got['lse'][0][r]} want {rec['lse']}"
        lp = float(got["logprob"][0][r])
        assert (lp == rec["logprob"]) if np.isinf(rec["logprob"]) else abs(lp - rec["logprob"]) <= bar, f"{what}: row {r} logprob"
        assert (got["topk_ids"][0][r].astype(np.int64) == rec["topk_ids"]).all(), f"{what}: row {r} ids {got['topk_ids'][0][r]}"
        want = rec["topk_logprob"]
        g = got["topk_logprob"][0][r].astype(np.float64)
        fin = np.isfinite(want)
        assert (np.abs(g[fin] - want[fin]) <= bar).all() and (g[~fin] == want[~fin]).all(), f"{what}: row {r} top-k logprobs"
    if k and live.size:
        picks = _argmax_rows(np.ascontiguousarray(x[live]), V)
        assert (got["topk_ids"][0][live, 0].astype(np.int64) == picks.reshape(-1).astype(np.int64)).all(), f"{what}: slot 0 is not the pick"
    return got


OP_SHAPES = [(8, 1), (8, 8), (257, 1), (257, 9), (320, 8), (320, 64), (4100, 3), (128256, 1), (128256, 8), (128256, 9), (128256, 64),
             (151936, 1), (151936, 64)]


@pytest.mark.parametrize("V,rows", OP_SHAPES, ids=[f"v{v}-r{r}" for v, r in OP_SHAPES])
def test_op_against_float64_and_the_pick(V, rows):
    for first_kind in (range(6) if rows == 1 else (0,)):    # (one row: the 64-slab layout of the single-sequence step sees every kind)
        x = _op_rows(V, rows, 1000 + V % 977 + rows, first_kind)
        tk = _op_tokens(V, rows, x)
        recs = {}
        for k in (8, 1, 0):
            _check_op(x, V, tk, min(k, V), f"V {V} rows {rows} kind {first_kind} k {k}", recs)


@pytest.mark.parametrize("V,rows,pad", [(257, 8, 3), (257, 8, 2), (320, 9, 4), (4100, 3, 5), (128256, 2, 4), (151936, 1, 3)])
def test_op_with_padding_behind_the_vocabulary(V, rows, pad):
    """ld > vocab with NaN in the padding.  A pitch that is a multiple of 4 keeps the 16-byte loads (257 + 3: with a one-element
    tail), the others take the element-wise trips; the numbers are the unpadded ones bit for bit either way."""
    from kjarni_amd import ops
    x = _op_rows(V, rows, 5 + V % 97)
    tk = _op_tokens(V, rows, x)
    xp = np.full((rows, V + pad), NAN, np.float32)
    xp[:, :V] = x
    got = _check_op(xp, V, tk, min(8, V), f"V {V} pad {pad}")
    plain = ops.token_logprobs(np.stack([x, x]), np.stack([tk, tk]), min(8, V), vocab=V)
    keep = tk >= 0
    for name in ("logprob", "lse", "topk_ids", "topk_logprob"):
        assert _same_bits(got[name][0][keep], plain[name][0][keep]), name


def test_op_lse_of_an_underflowing_row_is_the_maximum_and_top_k_zero():
    from kjarni_amd import ops
    V = 2049
    x = np.full((1, 1, V), -200.0, np.float32)
    x[0, 0, 1500] = 7.0
    got = ops.token_logprobs(x, [[1500]], 0)
    assert float(got["lse"][0, 0]) == 7.0 and float(got["logprob"][0, 0]) == 0.0 and got["slabs"] == 3
    assert got["topk_ids"].shape == (1, 1, 0)
    x[0, 0, :] = 1.5                                       # all equal: lse = x + log V
    got = ops.token_logprobs(x, [[0]], 2)
    assert abs(float(got["lse"][0, 0]) - (1.5 + np.log(V))) <= 2e-4 and got["topk_ids"][0, 0].tolist() == [V - 1, V - 2]


# ---- 2. the loops --------------------------------------------------------------------------------------------------------------------

def _raw_rows(ref, prompt, ids):
    """rows[i]: the float64 raw logits token ids[i] was decided from, i.e. the row behind prompt + ids[:i]."""
    if not len(ids):
        return np.zeros((0, ref.vocab))
    return np.asarray(ref.logits(list(prompt) + list(ids[:-1]), ref.new()), np.float64)[len(prompt) - 1:]


def _check_records(got, rows64, ids, k, what, bar_factor=1.0, cap=0.02):
    """got: dict with logprob [n], topk_ids / topk_logprob [n, k].  Returns (slots, slots left out); cap None: the caller sums
    them over the prompts of its case and asserts the cap there."""
    n = len(ids)
    assert got["logprob"].shape == (n,) and got["topk_ids"].shape == (n, k) and got["topk_logprob"].shape == (n, k), what
    if n == 0:
        return 0, 0
    want = R.run_record(rows64, ids, k)
    bar = bar_factor * 2.0 * TOL * max(1.0, float(np.abs(rows64[:n]).max()))
    err = float(np.abs(got["logprob"].astype(np.float64) - want["logprob"]).max())
    print(f"{what}: logprob err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got["logprob"]).all() and err <= bar, f"{what}: logprob {err:.3e} > {bar:.3e}"
    if k == 0:
        return 0, 0
    terr = float(np.abs(got["topk_logprob"].astype(np.float64) - want["topk_logprob"]).max())
    print(f"{what}: top-k logprob err {terr:.3e} bar {bar:.3e}")
    assert terr <= bar, f"{what}: top-k logprob {terr:.3e} > {bar:.3e}"
    clear = np.array([R.clear_slots(rows64[i], k, LC.GAP) for i in range(n)])
    left = int(clear.size - clear.sum())
    print(f"{what}: {left} of {clear.size} slots left out")
    if cap is not None:
        assert left <= (0 if clear.size < 50 else int(cap * clear.size)), f"{what}: {left} of {clear.size} slots lie within {LC.GAP} of a neighbour"
    assert (got["topk_ids"].astype(np.int64)[clear] == want["topk_ids"][clear]).all(), f"{what}: top-k ids"
    # the float64 log-probability of the id the device did choose is the value it returned
    lsm = np.array([R.log_softmax64(rows64[i])[got["topk_ids"][i].astype(np.int64)] for i in range(n)])
    assert float(np.abs(lsm - got["topk_logprob"]).max()) <= bar, f"{what}: a returned id does not carry its logprob"
    return int(clear.size), left


def _guard_intact(guard, entries, what):
    """guard: (ids, logprob, topk_ids, topk_logprob) behind a call's records, as the wrappers return them."""
    g_out, g_lp, g_ids, g_tlp = guard
    assert g_out.shape[0] == g_lp.shape[0] == g_ids.shape[0] == g_tlp.shape[0] == entries, what
    assert (g_out == 0xFFFFFFFF).all() and np.isnan(g_lp).all() and (g_ids == 0xFFFFFFFF).all() and np.isnan(g_tlp).all(), \
        f"{what}: entries behind the records were written"


def _family(tmp_path, family, seed, bf16=False, max_context=0):
    """(decoder, reference, config) of a tiny model; bf16: the matrices stored (and referenced) as bf16 values."""
    from kjarni_amd import HipDecoder
    d = str(tmp_path / f"{family}-{seed}-{int(bf16)}")
    if family == "gpt2":
        cfg = G.gpt2_config(**G.SMALL)
        _, t = G.gpt2_model(d, cfg, seed=seed, store_bf16=bf16)
        return HipDecoder(d, 0), SC.Gpt264(t, cfg), cfg
    if family == "qwen3":
        from tests import qwen3_fixture as Q3
        from tests.qwen3_ref64 import Qwen3Ref64
        cfg, t = Q3.qwen3_model(d, Q3.Q3_SMALL, seed=seed, store_bf16=bf16)
        return HipDecoder(d, 0), R.Qwen3Logits(Qwen3Ref64(t, cfg), cfg), cfg
    cfg, t = synth.llm_model(d, synth.LLAMA_TEST, seed=seed, store_bf16=bf16)
    return HipDecoder(d, max_context=max_context), SC.Llama64(t, cfg), cfg


def _prompt(ref, seed, n=6):
    return np.random.default_rng(seed).integers(ref.first_id, ref.vocab, n).tolist()


# (family, bf16) -> (model seed, prompt seed): tools/gen_logprobs_seed_search.py
GREEDY_SEEDS = {("llama", False): (1, 3), ("llama", True): (1, 1), ("gpt2", False): (1, 2), ("gpt2", True): (1, 3),
                ("qwen3", False): (1, 2), ("qwen3", True): (1, 3)}


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", ["llama", "gpt2", "qwen3"])
def test_plain_greedy_37_tokens_both_bursts(tmp_path, family, bf16):
    mseed, pseed = GREEDY_SEEDS[(family, bf16)]
    dec, ref, cfg = _family(tmp_path, family, mseed, bf16)
    prompt = _prompt(ref, pseed, 9)
    stops = [ref.vocab - 1]                                # (a stop id the runs do not meet: 37 tokens cross several bursts)
    base = dec.generate_sampled(prompt, 37, sample=False, stop_ids=stops)[0]
    assert len(base) == 37
    rows = _raw_rows(ref, prompt, base)
    seen = []
    for on_token, k in ((None, 8), (seen.append, 8), (None, 0), (None, 1)):
        got = dec.generate_logprobs(prompt, 37, top_k=k, stop_ids=stops, on_token=on_token)
        assert got["ids"] == base, (family, k)
        _check_records(got, rows, base, k, f"{family} bf16 {bf16} k {k} callback {on_token is not None}")
        if k:                                             # nothing edits the row: the emitted token is slot 0, bit for bit
            assert (got["topk_ids"][:, 0] == np.asarray(base)).all() and _same_bits(got["topk_logprob"][:, 0], got["logprob"])
    assert seen == base
    # generate, then score prompt + output: the same numbers inside twice the bar
    got = dec.generate_logprobs(prompt, 37, top_k=8, stop_ids=stops)
    lp, ids, tlp = dec.score_topk(prompt + base, first=len(prompt), top_k=8)
    bar = 2.0 * 2.0 * TOL * max(1.0, float(np.abs(rows).max()))
    assert float(np.abs(lp.astype(np.float64) - got["logprob"]).max()) <= bar
    assert float(np.abs(tlp.astype(np.float64) - got["topk_logprob"]).max()) <= bar
    assert dec.generate_sampled(prompt, 37, sample=False, stop_ids=stops)[0] == base      # a plain call afterwards: the ids it gave before
    assert dec.generate(prompt, 12) == dec.generate_logprobs(prompt, 12, top_k=2)["ids"]              # (the model's own stop ids)


SAMPLED = dict(temperature=0.8, sampling_top_k=12, top_p=None, min_p=0.02)


@pytest.mark.parametrize("family", ["llama", "gpt2"])
def test_processors_and_sampling_device_and_host(tmp_path, family):
    dec, ref, cfg = _family(tmp_path, family, 4 if family == "llama" else 1)
    prompt = _prompt(ref, 3, 7)
    n = 20
    u = np.random.default_rng(11).random(n).astype(np.float32)
    cases = {"penalty": dict(repetition_penalty=1.3, no_repeat_ngram=2),
             "sampled": dict(sample=True, uniforms=u, **SAMPLED),
             "sampled-penalty": dict(sample=True, uniforms=u, repetition_penalty=1.2, **SAMPLED)}
    for name, kw in cases.items():
        plain_kw = {("top_k" if key == "sampling_top_k" else key): v for key, v in kw.items()}
        plain_kw.setdefault("sample", False)
        for device in (True, False):
            dec.set_device_sampling(device)
            try:
                base = dec.generate_sampled(prompt, n, **plain_kw)[0]
                got = dec.generate_logprobs(prompt, n, top_k=5, **kw)
            finally:
                dec.set_device_sampling(True)
            assert got["ids"] == base and len(base) > 0, (name, device)
            rows = _raw_rows(ref, prompt, base)
            _check_records(got, rows, base, 5, f"{family} {name} device {device}")
            if name == "penalty":                        # the record is the RAW distribution: some emitted token is not slot 0
                assert (got["logprob"] <= got["topk_logprob"][:, 0] + 1e-6).all()


def test_constraint_and_grammar_record_the_raw_distribution(tmp_path):
    from kjarni_amd import constraints as K
    dec, ref, cfg = _family(tmp_path, "llama", 4, max_context=40)
    tokens = CC.model_tokens(cfg["vocab_size"])
    con = K.Constraint(r"[0-9]+", tokens)                 # digits only: it really masks
    prompt = _prompt(ref, 2, 6)
    n = 10
    u = np.random.default_rng(5).random(n).astype(np.float32)
    below = 0
    for name, kw in (("greedy", {}), ("greedy-callback", dict(on_token=lambda t: True)), ("penalty", dict(repetition_penalty=1.3)),
                     ("sampled", dict(sample=True, uniforms=u, **SAMPLED))):
        plain_kw = {("top_k" if key == "sampling_top_k" else key): v for key, v in kw.items()}
        for device in ((True, False) if name in ("penalty", "sampled") else (True,)):
            dec.set_device_sampling(device)
            try:
                base, res0 = dec.generate_constrained(con, prompt, n, **plain_kw)
                got = dec.generate_logprobs(prompt, n, top_k=4, constraint=con, **kw)
            finally:
                dec.set_device_sampling(True)
            assert got["ids"] == base and got["result"] == res0 and res0["violated"] == 0, (name, device)
            assert all(tokens[t].isdigit() for t in base) and len(base) > 0
            rows = _raw_rows(ref, prompt, base)
            _check_records(got, rows, base, 4, f"constraint {name} device {device}")
            below += int((got["logprob"] < got["topk_logprob"][:, 0] - 1e-3).sum())
    assert below > 0, "the mask never changed a pick: the case does not show that the raw row is recorded"
    gtokens = GC.model_tokens(cfg["vocab_size"])
    gram = K.GrammarConstraint(GC.rules_of(GC.LISTS), gtokens)
    for kw in ({}, dict(repetition_penalty=1.3)):
        base, res0 = dec.generate_grammar(gram, prompt, n, **kw)
        got = dec.generate_logprobs(prompt, n, top_k=4, grammar=gram, **kw)
        assert got["ids"] == base and got["result"] == res0 and len(base) > 0
        _check_records(got, _raw_rows(ref, prompt, base), base, 4, f"grammar {kw}")
    assert dec.generate(prompt, 8) == dec.generate_logprobs(prompt, 8, top_k=1)["ids"]


def test_endings(tmp_path):
    dec, ref, cfg = _family(tmp_path, "llama", 4, max_context=40)
    prompt = _prompt(ref, 23, 9)                          # (a prompt whose greedy run turns to a new token at step 4)
    free = dec.generate_sampled(prompt, 12, sample=False, stop_ids=[ref.vocab - 1])[0]
    rows = _raw_rows(ref, prompt, free)
    # a stop id is not emitted and has no record: the token of step 4 as the stop id
    stop = free[4]
    assert stop not in free[:4]
    got = dec.generate_logprobs(prompt, 12, top_k=3, stop_ids=[stop])
    assert got["ids"] == free[:4] and got["n"] == 4
    _check_records(got, rows, free[:4], 3, "stop id")
    # max_new_tokens
    got = dec.generate_logprobs(prompt, 7, top_k=3, stop_ids=[ref.vocab - 1])
    assert got["ids"] == free[:7]
    _check_records(got, rows, free[:7], 3, "max_new_tokens")
    # a callback that stops at token 3 (the third token is emitted, as generate() does it)
    seen = []
    got = dec.generate_logprobs(prompt, 12, top_k=3, stop_ids=[ref.vocab - 1], on_token=lambda t: seen.append(t) or len(seen) < 3)
    assert got["ids"] == free[:3] == seen
    _check_records(got, rows, free[:3], 3, "callback")
    # a full cache: 40 rows, a prompt of 33
    long_prompt = _prompt(ref, 8, 33)
    base = dec.generate_sampled(long_prompt, 20, sample=False, stop_ids=[ref.vocab - 1])[0]
    got = dec.generate_logprobs(long_prompt, 20, top_k=2, stop_ids=[ref.vocab - 1])
    assert got["ids"] == base and 0 < len(base) < 20
    _check_records(got, _raw_rows(ref, long_prompt, base), base, 2, "full cache")
    for device in (True, False):                          # ... and in the loops the host decides in
        dec.set_device_sampling(device)
        try:
            base = dec.generate_sampled(long_prompt, 20, sample=False, repetition_penalty=1.2, stop_ids=[ref.vocab - 1])[0]
            got = dec.generate_logprobs(long_prompt, 20, top_k=2, repetition_penalty=1.2, stop_ids=[ref.vocab - 1])
        finally:
            dec.set_device_sampling(True)
        assert got["ids"] == base and 0 < len(base) < 20
        _check_records(got, _raw_rows(ref, long_prompt, base), base, 2, f"full cache, penalty, device {device}")
    # capacity below n_out: the first `capacity` records, nothing behind them
    # (the wrapper allocates LOGPROB_GUARD entries behind the capacity it passes on, in all four arrays)
    from kjarni_amd.decoder import LOGPROB_GUARD
    got = dec.generate_logprobs(prompt, 12, top_k=3, stop_ids=[ref.vocab - 1], capacity=4)
    assert got["n"] == 12 and got["ids"] == free[:4]
    _check_records(got, rows, free[:4], 3, "capacity")
    _guard_intact(got["guard"], LOGPROB_GUARD, "capacity 4 below n_out 12")
    got = dec.generate_logprobs(prompt, 5, top_k=3, stop_ids=[ref.vocab - 1], capacity=9)
    assert got["n"] == 5
    _guard_intact(got["guard"], 4 + LOGPROB_GUARD, "capacity 9 above n_out 5")


def test_gguf_and_fp8_single_sequence(tmp_path):
    from kjarni_amd import HipDecoder
    from tests import fp8_fixture as F
    from tests import gguf_fixture as GG
    path, twin = str(tmp_path / "m" / "model.gguf"), str(tmp_path / "twin")
    types = {"embed": 8, "q": 12, "k": 8, "v": 12, "o": 8, "gate": 12, "up": 12, "down": 8}
    cfg, hf = GG.gguf_model(path, GG.LLAMA_Q, types, seed=3, rope_freqs=True, twin=twin)
    cases = [("gguf", HipDecoder(str(tmp_path / "m")), SC.Llama64(hf, cfg))]
    cfg8, hf8 = F.fp8_model(str(tmp_path / "fp8"), F.LLAMA_F8, "block", seed=1)
    cases.append(("fp8", HipDecoder(str(tmp_path / "fp8")), SC.Llama64(hf8, cfg8)))
    for name, dec, ref in cases:
        prompt = _prompt(ref, 7, 9)
        base = dec.generate_sampled(prompt, 16, sample=False, stop_ids=[ref.vocab - 1])[0]
        got = dec.generate_logprobs(prompt, 16, top_k=3, stop_ids=[ref.vocab - 1])
        assert got["ids"] == base and len(base) == 16, name
        _check_records(got, _raw_rows(ref, prompt, base), base, 3, name)


def test_refusals_on_the_device(tmp_path):
    import kjarni_amd
    from kjarni_amd import constraints as K
    dec, ref, cfg = _family(tmp_path, "llama", 4, max_context=40)
    prompt = _prompt(ref, 1, 6)
    before = dec.generate(prompt, 3)
    state = (dec.cache_len(), dec.resident())
    tokens = CC.model_tokens(cfg["vocab_size"])
    con = K.Constraint(r"[0-9]+", tokens)
    gram = K.GrammarConstraint(GC.rules_of(GC.LISTS), GC.model_tokens(cfg["vocab_size"]))
    for kw, word in ((dict(top_k=9), "top_k"), (dict(top_k=-1), "top_k"), (dict(top_k=2, constraint=con, grammar=gram), "not both"),
                     (dict(top_k=2, constraint=K.Constraint(r"a+", tokens[:100])), "token table")):
        with pytest.raises(kjarni_amd.KjarniException) as e:
            dec.generate_logprobs(prompt, 3, **kw)
        assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and word in str(e.value), kw
        assert (dec.cache_len(), dec.resident()) == state, kw
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_logprobs(list(range(4, 4 + 41)), 3, top_k=1)
    assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and "context" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        dec.generate_wide_logprobs([prompt, prompt], 3, top_k=9)
    assert e.value.code == kjarni_amd.KjarniError.INVALID_CONFIG and "top_k" in str(e.value)
    assert dec.generate(prompt, 3) == before


# ---- 3. lanes and wide ---------------------------------------------------------------------------------------------------------------

def _wide_case(tmp_path, case):
    from kjarni_amd import HipDecoder
    seed, cfg, t, ps, news = WC.case_set(case)
    d = str(tmp_path / case)
    WC.write_model(case, seed, d)
    ref = SC.Llama64(t, cfg)
    return HipDecoder(d, 0), ref, cfg, ps, news


@pytest.mark.parametrize("lanes", [3, 9, 64])
def test_generate_wide_logprobs_over_72_prompts(tmp_path, lanes):
    dec, ref, cfg, ps, news = _wide_case(tmp_path, "llama")
    base = dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT)
    got = dec.generate_wide_logprobs(ps, news, top_k=4, lanes=lanes, lane_context=WC.LANE_CONTEXT)
    assert [g["ids"] for g in got] == base
    assert len(ps) == 72 > lanes                          # every width turns lanes over: prompts enter lanes that ran another
    rows = [_raw_rows(ref, p, ids) for p, ids in zip(ps, base)]
    slots = left = 0
    for i, (g, r, ids) in enumerate(zip(got, rows, base)):
        assert len(ids) > 0
        s, l = _check_records(g, r, ids, 4, f"lanes {lanes} prompt {i}", cap=None)
        slots, left = slots + s, left + l
    assert left <= int(0.02 * slots), f"{left} of {slots} slots left out"
    # ... and against generate_logprobs of the prompt alone (another step kernel: inside twice the bar): every prompt, those of
    # the first round and those that entered a lane after turnover
    for i in range(len(ps)):
        one = dec.generate_logprobs(ps[i], news[i], top_k=4)
        assert one["ids"] == base[i]
        bar = 2.0 * 2.0 * TOL * max(1.0, float(np.abs(rows[i]).max()))
        assert float(np.abs(one["logprob"].astype(np.float64) - got[i]["logprob"]).max()) <= bar, i
        assert float(np.abs(one["topk_logprob"].astype(np.float64) - got[i]["topk_logprob"]).max()) <= bar, i
    assert dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT) == base
    # capacity below n_out (every prompt emits 4..10 tokens): the first 3 records of each, nothing behind any array
    from kjarni_amd.decoder import LOGPROB_GUARD
    few = dec.generate_wide_logprobs(ps, news, top_k=4, lanes=lanes, lane_context=WC.LANE_CONTEXT, capacity=3)
    assert all(len(b) > 3 for b in base)
    for i, g in enumerate(few):
        assert g["n"] == len(base[i]) and g["ids"] == base[i][:3], i
        for name in ("logprob", "topk_ids", "topk_logprob"):
            assert _same_bits(g[name], got[i][name][:3]), (i, name)
        _guard_intact(g["guard"], LOGPROB_GUARD if i == len(ps) - 1 else 0, f"lanes {lanes} capacity 3 prompt {i}")


def test_a_request_with_a_penalty_runs_in_a_batch(tmp_path):
    dec, ref, cfg, ps, news = _wide_case(tmp_path, "processors")
    ps, news = ps[:24], news[:24]
    for lanes in (4, 12):
        base = dec.generate_wide(ps, news, lanes=lanes, lane_context=WC.LANE_CONTEXT, **WC.PROCESSORS)
        got = dec.generate_wide_logprobs(ps, news, top_k=2, lanes=lanes, lane_context=WC.LANE_CONTEXT, **WC.PROCESSORS)
        assert [g["ids"] for g in got] == base
        slots = left = 0
        for i, (g, p, ids) in enumerate(zip(got, ps, base)):
            s, l = _check_records(g, _raw_rows(ref, p, ids), ids, 2, f"penalty lanes {lanes} prompt {i}", cap=None)
            slots, left = slots + s, left + l
        assert left <= int(0.02 * slots)


def test_moe_at_16_lanes(tmp_path):
    from kjarni_amd import HipDecoder
    from tests import moe_fixture as M
    from tests.moe_ref64 import MoeRef64
    d = str(tmp_path / "moe")
    cfg, t = M.moe_model(d, M.MOE_SMALL)
    dec = HipDecoder(d, 0)
    ps = WC.moe_prompts(cfg["vocab_size"])
    want = [WC.moe_clear_greedy(t, cfg, p, f"prompt {i}") for i, p in enumerate(ps)]
    got = dec.generate_wide_logprobs(ps, WC.MOE_NEW, top_k=2, lanes=16, lane_context=WC.LANE_CONTEXT)
    assert [g["ids"] for g in got] == want == dec.generate_wide(ps, WC.MOE_NEW, lanes=16, lane_context=WC.LANE_CONTEXT)
    ref = R.Qwen3Logits(MoeRef64(t, cfg), cfg)
    slots = left = 0
    for i, (g, p, ids) in enumerate(zip(got, ps, want)):
        s, l = _check_records(g, _raw_rows(ref, p, ids), ids, 2, f"moe prompt {i}", cap=None)
        slots, left = slots + s, left + l
    assert left <= int(0.02 * slots)


# ---- 4. the handles ------------------------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


def test_generator_and_chat_handles(tmp_path):
    import kjarni_amd
    from kjarni_amd import Chat, Generator, HipDecoder
    from kjarni_amd.chat import GenerationConfig
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen = Generator("gpt2", model_path=d)
    dec = HipDecoder(d, 0)
    greedy = GenerationConfig(do_sample=False, max_new_tokens=12)
    assert all(a.size == 0 for a in gen.last_logprobs())                  # zeros before any call
    plain = gen.generate(TEXTS[0], greedy)
    assert gen.last_logprobs()[0].size == 0                               # ... and after a call with logprobs off
    # Routed away from lookup and from a draft model: the plain loop.  Lookup and draft are lossless, so the text cannot tell; the
    # verify counters of the handle's model can: they move only when a call ran a verify step (lookup or draft loop).
    gen.set_logprobs(3)
    gen.set_prompt_lookup(4)
    v0 = gen.verify_gemv_calls()
    assert gen.generate(TEXTS[0], greedy) == plain and gen.verify_gemv_calls() == v0
    gen.set_draft_model(d, 3)                                             # (the same checkpoint as its own drafter)
    assert gen.generate(TEXTS[0], greedy) == plain and gen.verify_gemv_calls() == v0
    assert gen.last_logprobs()[0].size > 0
    gen.set_logprobs(None)                                                # ... and the counters are live: with records off both loops run
    assert gen.generate(TEXTS[0], greedy) == plain and sum(gen.verify_gemv_calls()) > sum(v0)
    v1 = gen.verify_gemv_calls()
    gen.set_draft_model(None, 0)
    assert gen.generate(TEXTS[0], greedy) == plain and sum(gen.verify_gemv_calls()) > sum(v1)
    gen.set_logprobs(3)
    v2 = gen.verify_gemv_calls()
    assert gen.generate(TEXTS[0], greedy) == plain and gen.verify_gemv_calls() == v2
    toks, lp, tt, tl = gen.last_logprobs()
    ids = gen.encode(TEXTS[0], greedy)
    one = dec.generate_logprobs(ids, 12, top_k=3)
    assert toks.tolist() == one["ids"] and _same_bits(lp, one["logprob"]) and _same_bits(tt, one["topk_ids"]) and _same_bits(tl, one["topk_logprob"])
    assert tt.shape == (len(one["ids"]), 3)
    pieces = []
    gen.stream(TEXTS[0], lambda s: pieces.append(s) or True, greedy)
    assert "".join(pieces) == plain and gen.last_logprobs()[0].tolist() == one["ids"]
    texts = gen.generate_batch(TEXTS, greedy)
    for i, text in enumerate(TEXTS):
        toks, lp, tt, tl = gen.last_logprobs(i)
        single = dec.generate_logprobs(gen.encode(text, greedy), 12, top_k=3)
        assert toks.tolist() == single["ids"] and tt.shape == (len(toks), 3), i
        assert float(np.abs(lp - single["logprob"]).max()) <= 4e-4 * max(1.0, float(np.abs(single["logprob"]).max())), i
    assert gen.last_logprobs(len(TEXTS))[0].size == 0                     # an index the call did not have
    gen.set_logprobs(0)
    assert gen.generate(TEXTS[1], greedy) is not None and gen.last_logprobs()[2].shape[1] == 0 and gen.last_logprobs()[1].size > 0
    with pytest.raises(kjarni_amd.KjarniException):
        gen.set_logprobs(9)
    gen.set_logprobs(None)                                                # off again
    gen.set_prompt_lookup(0)
    assert gen.generate(TEXTS[0], greedy) == plain and gen.last_logprobs()[0].size == 0
    assert texts == gen.generate_batch(TEXTS, greedy) and gen.last_logprobs(2)[0].size == 0
    gen.close()

    ld = str(tmp_path / "llama")
    synth.llm_model(ld, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(ld, "tokenizer.json"))
    chat = Chat("llama3.2-1b-instruct", model_path=ld)
    cfg = GenerationConfig(do_sample=False, max_new_tokens=10)
    assert chat.last_logprobs()[0].size == 0
    plain = chat.send("Is water wet?", cfg)
    chat.set_logprobs(2)
    chat.set_draft_model(ld, 3)                                           # routed away from the drafter while records are on
    c0 = chat.verify_gemv_calls()
    assert chat.send("Is water wet?", cfg) == plain and chat.verify_gemv_calls() == c0
    toks, lp, tt, tl = chat.last_logprobs()
    assert 0 < toks.size <= 10 and lp.shape == toks.shape and tt.shape == (toks.size, 2) and np.isfinite(lp).all()
    assert (tt[:, 0] == toks).all() and _same_bits(tl[:, 0], lp)          # plain greedy: the emitted token is slot 0
    assert (lp <= 0).all() and (tl[:, 0] >= tl[:, 1]).all()
    chat.set_logprobs(-1)
    assert chat.send("Is water wet?", cfg) == plain and chat.last_logprobs()[0].size == 0
    assert sum(chat.verify_gemv_calls()) > sum(c0)                        # (records off: the draft loop ran)
