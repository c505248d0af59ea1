"""Prefix reuse on the GPU (kjarni_hip_decoder_set_prefix_reuse and what sits on it).

Kept cache rows were computed by whichever route wrote them (a reply's rows by one-row decode steps, where a full prefill
takes the prompt GEMM), so nothing here is compared with a reuse-off run bit for bit: cache rows and logits are compared with
the float64 references under the decoder's bar, max |gpu - ref| <= 1e-4 * max(1, max |ref|) (tests/llm_ref64.py), and token
ids with the oracle's only on traces whose two best logits stay lanes_cases.GAP apart -- asserted here, on the CPU, before
the GPU is asked.  The lane copy is the exception: it moves bits, and is compared bit for bit.

The rule under test, stated once.  resident = the tokens behind cache rows [0, len(resident)).  A generate loop leaves
(prompt + emitted)[:cache_len]: every token it fed, and nothing of the rows it wrote for tokens it discarded.  A call with
reuse on keeps min(LCP(resident, prompt), limit) rows, limit = len(prompt) - 1 for the generate loops (the last prompt
token's logits are needed) and first - 1 for score (rows first - 1 .. n - 2 must reach the head)."""
import os
import shutil

import numpy as np
import pytest

from oracle import llm_oracle as L
from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import llm_ref64, synth
from tests import lookup_cases as LK
from tests import sampled_lookup_cases as S

pytestmark = pytest.mark.gpu
TOL = llm_ref64.TOL
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
QK = 2.0          # peaked attention (tests/test_gpu_llm_cache.py): a stale or misplaced row shows
SAMPLED = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05)


def _bar(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _lcp(a, b):
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return n


def _check(dec, ref, tokens, what, logits=False):
    """Cache rows [0, len(tokens)) of every layer, and optionally the logits the device holds, against float64 on `tokens`."""
    cache = ref.new()
    want = ref.logits(tokens, cache)
    n = len(tokens)
    assert dec.cache_len() >= n, (what, dec.cache_len(), n)
    got = [dec.kv_rows(i, 0, n) for i in range(len(cache))]
    for (layer, name), (err, bar) in sorted(llm_ref64.cache_errors(got, cache).items()):
        print(f"{what}: layer {layer} {name} err {err:.3e} bar {bar:.3e}")
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e} (first bad row " \
                           f"{llm_ref64.first_bad_row(got[layer]['kv'.index(name)], cache[layer]['kv'.index(name)], bar)})"
    if logits:
        lg = dec.last_logits()
        err, bar = float(np.abs(lg.astype(np.float64) - want[-1]).max()), _bar(want[-1])
        print(f"{what}: logits err {err:.3e} bar {bar:.3e}")
        assert np.isfinite(lg).all() and err <= bar, f"{what}: logits {err:.3e} > {bar:.3e}"


def _trace64(ref, prompt, n):
    """n greedy tokens of the float64 reference (the last maximum wins) and the smallest gap between its two best logits."""
    cache = ref.new()
    row = ref.logits(prompt, cache)[-1]
    out, gap = [], float("inf")
    for _ in range(n):
        top = np.partition(row, -2)[-2:]
        gap = min(gap, float(top[1] - top[0]))
        out.append(int(len(row) - 1 - np.argmax(row[::-1])))
        row = ref.logits([out[-1]], cache)[-1]
    return out, gap


def _delta(dec, before):
    r, c = dec.prefix_stats()
    return r - before[0], c - before[1]


# ---- the models ------------------------------------------------------------------------------------------------------------------

def _llama(tmp_path, base, seed, name="m", **kw):
    import kjarni_amd
    d = str(tmp_path / name)
    ctx = kw.pop("max_context", 0)
    cfg, t = synth.llm_model(d, base, seed=seed, **kw)
    return kjarni_amd.HipDecoder(d, max_context=ctx), t, cfg


def _pair(tmp_path, kind):
    """(decoder, float64 reference) of one of the stacks reuse must work on."""
    from kjarni_amd import HipDecoder
    if kind == "gpt2":
        cfg = G.gpt2_config(**G.SMALL)
        d = str(tmp_path / "gpt2")
        _, t = G.gpt2_model(d, cfg, seed=1)
        return HipDecoder(d, 0), S.Gpt264(t, cfg)
    if kind == "gguf-q8_0":
        path = str(tmp_path / "m" / "model.gguf")
        cfg, hf = GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
        dec = HipDecoder(str(tmp_path / "m"))
        by = dec.weight_bytes_by_type()
        assert by.get("Q8_0", 0) > 0 and "Q4_K" not in by and "Q6_K" not in by
        return dec, S.Llama64(hf, dict(cfg, model_type="llama"))
    base, kw = {"llama": (synth.LLAMA_TEST, {}), "qwen2": (synth.QWEN_TEST, {}), "bf16": (synth.LLAMA_TEST, dict(store_bf16=True))}[kind]
    dec, t, cfg = _llama(tmp_path, base, 3, qk_scale=QK, **kw)
    assert dec.bf16 == (kind == "bf16")
    return dec, S.Llama64(t, cfg)


# ---- 1. rows after reuse ---------------------------------------------------------------------------------------------------------

def _fresh_ids(rng, ref, n, avoid):
    ids = rng.integers(ref.first_id, min(ref.vocab, 700), n).tolist()     # (700: GPT-2's <|endoftext|>)
    if ids[0] == avoid:
        ids[0] = ref.first_id + (avoid - ref.first_id + 1) % (min(ref.vocab, 700) - ref.first_id)
    return ids


@pytest.mark.parametrize("kind", ["llama", "qwen2", "gpt2", "bf16", "gguf-q8_0"])
def test_rows_after_reuse(tmp_path, kind):
    """37 resident tokens, then a prompt that shares the first 20: the call keeps 20 rows and computes the rest -- 1 row (the
    one-row fused step at pos 20), 5 rows (an 8-row pass at row_off 20), 40 rows (the prompt GEMM with base 20) -- and every row
    of the cache, the kept ones and the new ones, is the float64 reference's row of the new prompt; nothing of the old 37 is
    left behind the kept length.  Then shrinking: a 9-token prefix of the resident tokens keeps 8 rows and computes 1."""
    dec, ref = _pair(tmp_path, kind)
    rng = np.random.default_rng(5)
    A = rng.integers(ref.first_id, min(ref.vocab, 700), 37).tolist()
    dec.set_prefix_reuse(True)
    for suffix in (1, 5, 40):
        B = A[:21] if suffix == 1 else A[:20] + _fresh_ids(rng, ref, suffix, avoid=A[20])
        assert _lcp(A, B) == (21 if suffix == 1 else 20)
        dec.reset()
        assert dec.resident() == []
        dec.forward(A, fetch=False)
        assert dec.resident() == A
        before = dec.prefix_stats()
        assert dec.generate(B, 0) == []
        assert _delta(dec, before) == (20, len(B) - 20), suffix
        assert dec.resident() == B and dec.cache_len() == len(B)
        _check(dec, ref, B, f"{kind} suffix {suffix}", logits=True)
    # shrinking
    dec.reset()
    dec.forward(A, fetch=False)
    before = dec.prefix_stats()
    assert dec.generate(A[:9], 0) == []
    assert _delta(dec, before) == (8, 1)
    assert dec.resident() == A[:9] and dec.cache_len() == 9
    _check(dec, ref, A[:9], f"{kind} shrink", logits=True)
    # and growing again from what is left: 9 kept, the rest computed on top
    before = dec.prefix_stats()
    assert dec.generate(A, 0) == []
    assert _delta(dec, before) == (9, 28)
    _check(dec, ref, A, f"{kind} regrow", logits=True)


# ---- 2. what the loops leave ---------------------------------------------------------------------------------------------------

SIX = [201, 17, 88, 133, 250, 64]


def _eos_case():
    """The many-stops model: (prompts, max_new per prompt): one run that ends on a stop id inside a burst, one that ends on
    max_new.  Both turns' oracle traces must clear the gap."""
    cfg, t = dict(LC.EOS_BASE), synth.llm_tensors(dict(LC.EOS_BASE), LC.EOS_SEED)
    orc = L.LlmOracle(t, cfg)
    ps = LC.prompts(LC.EOS_SEED, cfg["vocab_size"])
    ends = LC.stop_steps(orc, ps, LC.MAX_NEW)
    stopped = [i for i, s in sorted(ends.items()) if 2 <= s and s % 16 != 0]   # the stop id is not the last token of a burst
    free = [i for i in range(len(ps)) if i not in ends]
    assert stopped and free, "precondition: a prompt that stops inside a burst and one that does not stop"
    return orc, [(ps[stopped[0]], LC.MAX_NEW, "stop"), (ps[free[0]], 9, "max_new")]


def _two_turns(orc, p1, new1, new2=12, **kw):
    """(out1, p2, out2) of the oracle, the gap of both traces asserted."""
    (e1,), gap1 = LC.oracle_runs(orc, [p1], new1, **kw)
    p2 = list(p1) + e1 + SIX
    (e2,), gap2 = LC.oracle_runs(orc, [p2], new2, **kw)
    assert min(gap1, gap2) >= LC.GAP, f"precondition: the oracle's two best logits come within {min(gap1, gap2):.2e}"
    return e1, p2, e2


def _after_turn(dec, ref, p, out, what):
    """The rule: the loop leaves (p + out)[:cache_len], at most one token short of p + out; those rows are the reference's."""
    whole = list(p) + list(out)
    res = dec.resident()
    assert res == whole[:min(len(whole), dec.cache_len())], what
    assert len(res) >= len(whole) - 1, what
    _check(dec, ref, res, what)
    return res


@pytest.mark.parametrize("loop", ["generate", "lookup"])
def test_greedy_loops_leave_the_fed_tokens(tmp_path, loop):
    """Turn 1 generates; turn 2's prompt is turn 1's prompt + its output + six new ids.  The plain loop runs bursts of 16
    steps: a stop id inside a burst leaves up to 15 rows of discarded tokens behind, which must not count.  Ended by a stop
    id, every emitted token was fed (the stop id came out of the last one's row): resident = prompt + output, and turn 2 keeps
    all of it.  Ended by max_new, the last token was not fed: turn 2 keeps one less."""
    orc, cases = _eos_case()
    dec, t, cfg = _llama(tmp_path, LC.EOS_BASE, LC.EOS_SEED)
    ref = S.Llama64(t, cfg)
    dec.set_prefix_reuse(True)
    run = (lambda p, n: dec.generate(p, n)) if loop == "generate" else (lambda p, n: dec.generate_lookup(p, n)[0])
    for p1, new1, how in cases:
        e1, p2, e2 = _two_turns(orc, p1, new1)
        assert (len(e1) < new1) == (how == "stop")
        dec.reset()
        before = dec.prefix_stats()
        assert run(p1, new1) == e1
        assert _delta(dec, before) == (0, len(p1))
        res = _after_turn(dec, ref, p1, e1, f"{loop} {how} turn 1")
        if loop == "generate":
            assert len(res) == len(p1) + len(e1) - (0 if how == "stop" else 1)
            if how == "stop":
                assert dec.cache_len() > len(res), "precondition: the burst ran past the stop id"
        before = dec.prefix_stats()
        assert run(p2, 12) == e2
        assert _delta(dec, before) == (len(res), len(p2) - len(res)), (loop, how)
        _after_turn(dec, ref, p2, e2, f"{loop} {how} turn 2")


def test_processors_count_the_reused_tokens(tmp_path):
    """A greedy run with repetition_penalty 1.3 and a 2-gram ban on both turns: the history and the token counts of turn 2 are
    built from the whole prompt, not from the suffix that was forwarded -- the ids are the oracle's."""
    kw = dict(repetition_penalty=1.3, no_repeat_ngram=2)
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, LC.PROCESSOR_SEED)
    orc, ref = L.LlmOracle(t, cfg), S.Llama64(t, cfg)
    p1 = LC.prompts(LC.PROCESSOR_SEED, cfg["vocab_size"])[1]
    e1, p2, e2 = _two_turns(orc, p1, 10, **kw)
    plain = orc.generate(p2, 12)
    assert plain != e2, "precondition: the processors change turn 2's ids"
    assert len(e1) == 10
    dec.set_prefix_reuse(True)
    assert dec.generate(p1, 10, **kw) == e1
    res = _after_turn(dec, ref, p1, e1, "processors turn 1")
    assert len(res) == len(p1) + len(e1) - 1          # the loop ends at its length cap before it feeds the last token
    before = dec.prefix_stats()
    assert dec.generate(p2, 12, **kw) == e2
    assert _delta(dec, before) == (len(res), len(p2) - len(res))
    _after_turn(dec, ref, p2, e2, "processors turn 2")


def _sampled_case(ref, cfg):
    """Two turns of the float64 sampler on steered draws (tests/sampled_lookup_cases.py: every filter decision and every draw
    clears its boundary by the margin, so a deviation inside the float bar cannot change a token)."""
    eos = tuple(cfg["eos_token_id"])
    rng = np.random.default_rng(1)
    why = None
    for _ in range(8):
        a = rng.integers(ref.first_id, ref.vocab, 5).tolist()
        p1 = a + a[:4] + rng.integers(ref.first_id, ref.vocab, 2).tolist() + a[:2]
        try:
            tr1 = S.build_trace(ref, p1, 12, SAMPLED, avoid=eos)
            p2 = p1 + tr1.ids + SIX
            tr2 = S.build_trace(ref, p2, 12, SAMPLED, avoid=eos)
        except AssertionError as e:
            why = e
            continue
        if len(tr1.ids) == 12 and len(tr2.ids) == 12:
            return p1, tr1, p2, tr2
    raise AssertionError(f"precondition: none of the seeded prompts gives two clear traces ({why})")


@pytest.mark.parametrize("lookup", [None, LK.DEFAULT], ids=["plain", "lookup"])
def test_sampled_loops_leave_the_fed_tokens(tmp_path, lookup):
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, 4)
    ref = S.Llama64(t, cfg)
    p1, tr1, p2, tr2 = _sampled_case(ref, cfg)
    kw = {k: SAMPLED.get(k) for k in ("temperature", "top_k", "top_p", "min_p")}
    off1, _ = dec.generate_sampled(p1, 12, lookup=lookup, uniforms=tr1.uniforms, **kw)          # reuse off: today's run
    off2, _ = dec.generate_sampled(p2, 12, lookup=lookup, uniforms=tr2.uniforms, **kw)
    assert off1 == tr1.ids and off2 == tr2.ids and dec.prefix_stats() == (0, 0)
    dec.reset()
    dec.set_prefix_reuse(True)
    got1, _ = dec.generate_sampled(p1, 12, lookup=lookup, uniforms=tr1.uniforms, **kw)
    assert got1 == off1
    res = _after_turn(dec, ref, p1, got1, f"sampled {lookup} turn 1")
    # both loops end at the length cap with their last pick not fed
    assert len(res) == len(p1) + 12 - 1
    before = dec.prefix_stats()
    got2, _ = dec.generate_sampled(p2, 12, lookup=lookup, uniforms=tr2.uniforms, **kw)
    assert _delta(dec, before) == (len(res), len(p2) - len(res))
    assert got2 == off2
    _after_turn(dec, ref, p2, got2, f"sampled {lookup} turn 2")


# ---- 3. score ------------------------------------------------------------------------------------------------------------------

def _check_score(got, ref, ids, first, what):
    """test_gpu_score.py's bars: logprob and top_logprob within 2B, B the logits' bar; the arg-max on rows with a clear gap."""
    lp, top, tlp = got
    cache = ref.new()
    lg = ref.logits(ids, cache)[first - 1:len(ids) - 1]
    mx = lg.max(axis=1, keepdims=True)
    lsm = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
    rows = np.arange(lg.shape[0])
    want_top = (lg.shape[1] - 1 - np.argmax(lg[:, ::-1], axis=1))
    bar = 2.0 * _bar(lg)
    for name, g, w in (("logprob", lp, lsm[rows, np.asarray(ids[first:], np.int64)]), ("top_logprob", tlp, lsm[rows, want_top])):
        err = float(np.abs(np.asarray(g, np.float64) - w).max())
        print(f"{what}: {name} err {err:.3e} bar {bar:.3e}")
        assert g.shape == (len(ids) - first,) and np.isfinite(g).all() and err <= bar, f"{what}: {name}: {err:.3e} > {bar:.3e}"
    part = np.partition(lg, -2, axis=1)[:, -2:]
    clear = (part[:, 1] - part[:, 0]) >= LC.GAP
    assert (top[clear].astype(np.int64) == want_top[clear]).all(), f"{what}: arg-max"


@pytest.mark.parametrize("fused", [True, False], ids=["fused-head", "rows-head"])
def test_score_reuses_the_context(tmp_path, fused):
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, 3, qk_scale=QK)
    ref = S.Llama64(t, cfg)
    rng = np.random.default_rng(8)
    ctx = rng.integers(4, cfg["vocab_size"], 30).tolist()
    c1, c2, c3 = ([int(x) for x in rng.integers(4, cfg["vocab_size"], n)] for n in (5, 4, 26))
    c2[0] = c1[0] + 1 if c1[0] + 1 < cfg["vocab_size"] else 4
    c3[0] = c2[0]
    c3[1] = c2[1] + 1 if c2[1] + 1 < cfg["vocab_size"] else 4
    dec.set_score_fused(fused)
    dec.set_prefix_reuse(True)
    first = len(ctx)
    # (ids, first, rows kept): a fresh cache; the context shared; the context and one continuation token shared (the limit
    # first - 1 still holds the call to 29 rows: 26 + 1 rows go through the prompt GEMM at base 29); first far inside the shared
    # part (first - 1 = 9 < LCP: 9 rows kept, 25 computed); the same sequence again (limit first - 1, not n - 1)
    calls = [(ctx + c1, first, 0), (ctx + c2, first, 29), (ctx + c3, first, 29), (ctx + c2, 10, 9), (ctx + c2, first, 29)]
    for i, (ids, f, keep) in enumerate(calls):
        before = dec.prefix_stats()
        want_keep = min(_lcp(dec.resident(), ids), f - 1)
        assert want_keep == keep, i
        got = dec.score(ids, f)
        assert _delta(dec, before) == (keep, len(ids) - keep), i
        assert dec.resident() == ids and dec.cache_len() == len(ids)
        _check_score(got, ref, ids, f, f"score call {i} (kept {keep})")
        _check(dec, ref, ids, f"score call {i}")
    fused_calls, rows_calls = dec.score_calls()
    assert (fused_calls > 0 and rows_calls == 0) if fused else (fused_calls == 0 and rows_calls > 0)
    # a generate call after a score call reuses the scored sequence
    before = dec.prefix_stats()
    dec.generate(ctx + c2 + [9], 0)
    assert _delta(dec, before) == (len(ctx + c2), 1)


# ---- 4. off is off ---------------------------------------------------------------------------------------------------------------

def test_off_is_off_and_the_switch_moves_between_calls(tmp_path):
    base = dict(synth.LLAMA_TEST, eos_token_id=[])          # no stop id: all tokens come (tests/test_gpu_llm_cache.py)
    dec, t, cfg = _llama(tmp_path, base, 11, qk_scale=QK)
    ref = S.Llama64(t, cfg)
    prompt = np.random.default_rng(111).integers(4, cfg["vocab_size"], 30).tolist()
    want, gap = _trace64(ref, prompt, 20)
    assert gap >= LC.GAP, f"precondition: {gap:.2e}"
    for _ in range(2):                                      # the switch never set
        assert dec.generate(prompt, 20) == want
        assert dec.prefix_stats() == (0, 0)
        assert dec.cache_len() == len(prompt) + 20 - 1      # what generate() has always left: the last token is not fed
        assert dec.resident() == prompt + want[:-1]         # tracked all the same, so that switching on works mid-session
    lp = dec.score(prompt, 1)
    assert dec.prefix_stats() == (0, 0) and dec.resident() == prompt
    dec.set_prefix_reuse(True)                              # on: the scored prompt is resident
    assert dec.generate(prompt, 20) == want
    assert dec.prefix_stats() == (len(prompt) - 1, 1)
    _check(dec, ref, prompt + want[:-1], "switched on")
    dec.set_prefix_reuse(False)                             # off again: a full prefill, the counters stand still
    assert dec.generate(prompt, 20) == want
    assert dec.prefix_stats() == (len(prompt) - 1, 1) and dec.cache_len() == len(prompt) + 19
    dec.set_prefix_reuse(True)                              # and on: the run before left its tokens
    assert dec.generate(prompt + want[:5], 15) == want[5:]
    assert dec.prefix_stats() == (2 * len(prompt) - 1 + 4, 2)
    dec.reset()
    assert dec.resident() == [] and dec.cache_len() == 0
    assert dec.generate(prompt, 20) == want                 # an empty cache: everything is computed
    assert dec.prefix_stats() == (2 * len(prompt) - 1 + 4, 2 + len(prompt))
    assert np.array_equal(lp[1], dec.score(prompt, 1)[1])
    # hooks that do not say what they fed end the tracked prefix; forward() after them must not pretend otherwise
    dec.reset()
    dec.forward(prompt[:10], fetch=False)
    dec.verify_step(prompt[10], [prompt[11]], 2)
    dec.forward(prompt[:3], fetch=False)
    assert dec.resident() == prompt[:10] and dec.cache_len() > 10


# ---- 5. the lane copy ------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_copy_kernel_alone_is_bit_exact_at_every_alignment():
    """launch_kv_prefix_copy on buffers whose source, destination and destination offset break the 16-byte alignment in every
    combination, with counts that are no multiple of 4, below one vector, and past one trip of the whole grid (256 blocks x
    256 threads x 4 floats = 262 144): every bit pattern (NaN payloads, denormals) arrives, and nothing else is written."""
    from kjarni_amd import ops
    rng = np.random.default_rng(0)
    layers, src_floats, dst_floats = 2, 700, 1500
    src = rng.integers(0, 2 ** 32, (2 * layers, src_floats), dtype=np.uint64).astype(np.uint32).view(np.float32)
    dst = rng.integers(0, 2 ** 32, (2 * layers, dst_floats), dtype=np.uint64).astype(np.uint32).view(np.float32)
    done = 0
    for ss in range(4):
        for ds in range(4):
            for off in (0, 1, 6, 799):
                for count in (0, 1, 3, 4, 5, 257, 700):
                    out = ops.kv_prefix_copy(src, dst, off, count, src_skew=ss, dst_skew=ds)
                    want = _bits(dst).copy()
                    want[:, off:off + count] = _bits(src)[:, :count]
                    assert np.array_equal(_bits(out), want), (ss, ds, off, count)
                    done += 1
    assert done == 448
    big = 300001
    src = rng.integers(0, 2 ** 32, (2, big), dtype=np.uint64).astype(np.uint32).view(np.float32)
    dst = np.zeros((2, big + 9), np.float32)
    for ss, ds, off in ((0, 0, 0), (0, 0, 4), (1, 1, 0), (0, 2, 3), (3, 0, 8), (0, 1, 3)):   # (the last: skew and offset cancel)
        out = ops.kv_prefix_copy(src, dst, off, big, src_skew=ss, dst_skew=ds)
        want = _bits(dst).copy()
        want[:, off:off + big] = _bits(src)
        assert np.array_equal(_bits(out), want), (ss, ds, off)
    with pytest.raises(Exception, match="outside"):
        ops.kv_prefix_copy(src, dst, 10, big)               # 10 + count > the destination
    with pytest.raises(Exception, match="outside"):
        ops.kv_prefix_copy(src, dst, 0, big + 1)            # count > the source


KV8 = dict(synth.LLAMA_TEST, num_attention_heads=8, num_key_value_heads=1, head_dim=8)


@pytest.mark.parametrize("kind", ["kv8", "kv32", "gpt2-kv64"])
def test_lane_copy_alone(tmp_path, kind):
    """After forward of 19 ids: lanes_begin(3) with `cap` rows per lane (24; 25 at kv 8: an odd capacity at the narrowest
    rows), lanes 0 and 1 filled, then lane 2 takes the first s rows of the single-sequence cache and prefills a suffix behind
    them.  s = 1, 19 and capacity - 1.  The copied rows equal the source bit for bit, the suffix rows are the reference's, a
    step on the lane attends over both, and the other lanes, the single-sequence cache and resident() are untouched.
    A lane's offset is lane x capacity x kv floats and kv = kv_heads x head_dim is a multiple of 4 on every model the loader
    takes (test_loader_refuses_rows_that_would_unalign_a_lane), so these copies take the 16-byte path; the 4-byte path is
    test_copy_kernel_alone_is_bit_exact_at_every_alignment's."""
    cap = 25 if kind == "kv8" else 24
    if kind == "gpt2-kv64":
        dec, ref = _pair(tmp_path, "gpt2")
    else:
        dec, t, cfg = _llama(tmp_path, KV8 if kind == "kv8" else synth.LLAMA_TEST, 3, qk_scale=QK)
        ref = S.Llama64(t, cfg)
        assert dec.kv_heads * dec.head_dim == (8 if kind == "kv8" else 32)
    rng = np.random.default_rng(9)
    hi = min(ref.vocab, 700)
    main = rng.integers(ref.first_id, hi, cap - 1).tolist()
    dec.forward(main[:19], fetch=False)
    for s, n_suffix in ((1, 3), (19, 4), (cap - 1, 1)):
        if s > dec.cache_len():
            dec.forward(main[19:], fetch=False)
        held = dec.cache_len()
        dec.lanes_begin(3, cap)
        assert dec.lane_capacity() == cap
        others = [rng.integers(ref.first_id, hi, n).tolist() for n in (cap, 7)]
        for lane, ids in enumerate(others):
            dec.lane_prefill(lane, ids)
        snap = [[dec.lane_kv_rows(lane, layer) for layer in range(dec.layers)] for lane in (0, 1)]
        main_rows = [dec.kv_rows(layer) for layer in range(dec.layers)]
        suffix = rng.integers(ref.first_id, hi, n_suffix).tolist()
        dec.lane_prefill_shared(2, s, suffix)
        assert dec.lane_cache_len(2) == s + n_suffix and dec.cache_len() == held and dec.resident() == main[:held]
        cache = ref.new()
        ref.logits(main[:s] + suffix, cache)
        for layer in range(dec.layers):
            k, v = dec.lane_kv_rows(2, layer, 0, s)
            assert np.array_equal(_bits(k), _bits(main_rows[layer][0][:s])) and np.array_equal(_bits(v), _bits(main_rows[layer][1][:s])), (s, layer)
            got = dec.lane_kv_rows(2, layer, s, n_suffix)
            for g, w, name in zip(got, cache[layer], "kv"):
                err, bar = float(np.abs(g - w[s:]).max()), _bar(w)
                assert err <= bar, f"{kind} s {s} layer {layer} {name} suffix rows: {err:.3e} > {bar:.3e}"
            for lane in (0, 1):
                for a, b in zip(dec.lane_kv_rows(lane, layer), snap[lane][layer]):
                    assert np.array_equal(_bits(a), _bits(b)), (s, lane, layer)
            for a, b in zip(dec.kv_rows(layer), main_rows[layer]):
                assert np.array_equal(_bits(a), _bits(b)), (s, layer)
        if s + n_suffix < cap:                              # one lock-step step on lane 2 alone: it attends over copied + new rows
            tok = int(rng.integers(ref.first_id, hi))
            _, logits = dec.lanes_step([0, 0, tok], live=[0, 0, 1])
            want = ref.logits([tok], cache)[-1]
            err = float(np.abs(logits[2] - want).max())
            assert err <= _bar(want), f"{kind} s {s}: step logits {err:.3e}"
    with pytest.raises(Exception, match="shared prefix"):
        dec.lane_prefill_shared(2, dec.cache_len() + 1, [5])
    with pytest.raises(Exception, match="does not fit"):
        dec.lane_prefill_shared(2, cap - 1, [5, 6])
    with pytest.raises(Exception, match="no such lane"):
        dec.lane_prefill_shared(3, 1, [5])


def test_loader_refuses_rows_that_would_unalign_a_lane(tmp_path):
    """A lane offset can leave the 16-byte grid only with kv = kv_heads x head_dim off a multiple of 4 floats, which needs a
    head_dim that is no multiple of 4: hidden 48 as 8 heads of 6 over 1 KV head would put lane 1 of a 25-row lane at 150 floats =
    600 bytes.  LlmModel::load refuses such a head_dim (the attention kernels take 4, 8, ... 128) before anything reaches the
    device, so no model brings an unaligned lane to the copy."""
    import kjarni_amd
    base = dict(synth.LLAMA_TEST, hidden_size=48, num_attention_heads=8, num_key_value_heads=1, head_dim=6, intermediate_size=96)
    d = str(tmp_path / "d6")
    synth.llm_model(d, base, seed=3)
    with pytest.raises(Exception, match="unsupported decoder geometry"):
        kjarni_amd.HipDecoder(d)
    cfg = G.gpt2_config(**dict(G.SMALL, n_embd=72, n_head=12))     # GPT-2: rows of hidden floats, heads of 6
    g = str(tmp_path / "gpt2-d6")
    G.gpt2_model(g, cfg, seed=1)
    with pytest.raises(Exception, match="unsupported decoder geometry"):
        kjarni_amd.HipDecoder(g)


# ---- 6. lanes end to end ---------------------------------------------------------------------------------------------------------

SUFFIX_LENS = (1, 3, 6, 9, 12)
NEWS = [5, 9, 3, 12, 7]


def _lanes_case(cfg):
    rng = np.random.default_rng(21)
    shared = rng.integers(4, cfg["vocab_size"], 19).tolist()
    tails, first = [], set()
    for n in SUFFIX_LENS:                                   # the suffixes differ in their first id: the shared prefix is the 19 ids
        tail = rng.integers(4, cfg["vocab_size"], n).tolist()
        while tail[0] in first:
            tail[0] = 4 + (tail[0] - 3) % (cfg["vocab_size"] - 4)
        first.add(tail[0])
        tails.append(tail)
    return shared, [shared + tail for tail in tails]


@pytest.mark.parametrize("kw", [{}, dict(repetition_penalty=1.3, no_repeat_ngram=2)], ids=["greedy-graph", "processors"])
def test_lanes_share_the_prefix(tmp_path, kw):
    """5 requests that share 19 ids, on 3 lanes, so that two of them enter as refills between bursts.  The ids are the oracle's
    (requests with processors take the uncaptured lane path: only their prefill changes).  computed counts what was run through
    the model: the shared prefix once, every request's suffix; a second call finds the prefix resident."""
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, 7)
    orc = L.LlmOracle(t, cfg)
    shared, ps = _lanes_case(cfg)
    exp, gap = LC.oracle_runs(orc, ps, NEWS, **kw)
    assert gap >= LC.GAP, f"precondition: {gap:.2e}"
    assert [len(e) for e in exp] == NEWS, "precondition: no request ends on a stop id"
    assert dec.generate_batch(ps, NEWS, lanes=3, lane_context=64, **kw) == exp and dec.prefix_stats() == (0, 0)   # off: today's call
    dec.reset()
    dec.set_prefix_reuse(True)
    tails = sum(len(p) - 19 for p in ps)
    assert dec.generate_batch(ps, NEWS, lanes=3, lane_context=64, **kw) == exp
    assert dec.prefix_stats() == (5 * 19, 19 + tails)
    assert dec.resident() == shared and dec.cache_len() == 19      # the prefix stays in the single-sequence cache
    before = dec.prefix_stats()
    assert dec.generate_batch(ps, NEWS, lanes=3, lane_context=64, **kw) == exp
    assert _delta(dec, before) == (19 + 5 * 19, tails)             # the second call computes only the suffixes
    # one request is exactly the 19 ids: its last token must be forwarded for its logits, so 18 are shared
    ps6, news6 = ps + [shared], NEWS + [6]
    exp6, gap = LC.oracle_runs(orc, ps6, news6, **kw)
    assert gap >= LC.GAP and exp6[:5] == exp
    before = dec.prefix_stats()
    assert dec.generate_batch(ps6, news6, lanes=3, lane_context=64, **kw) == exp6
    assert _delta(dec, before) == (18 + 6 * 18, sum(len(p) - 18 for p in ps6))
    assert dec.resident() == shared[:18]
    # a single-sequence call afterwards starts from the resident prefix
    before = dec.prefix_stats()
    assert dec.generate(ps[1], NEWS[1], **kw) == exp[1]
    assert _delta(dec, before) == (18, len(ps[1]) - 18)


def test_identical_prompts_in_lanes(tmp_path):
    dec, t, cfg = _llama(tmp_path, synth.LLAMA_TEST, 7)
    orc = L.LlmOracle(t, cfg)
    p = _lanes_case(cfg)[1][3]
    (e,), gap = LC.oracle_runs(orc, [p], 10)
    assert gap >= LC.GAP and len(e) == 10
    dec.set_prefix_reuse(True)
    assert dec.generate_batch([p] * 4, 10, lanes=4, lane_context=64) == [e] * 4
    assert dec.prefix_stats() == (4 * (len(p) - 1), len(p) + 3)
    # a request that never enters a lane (nothing to generate) does not cost the others their shared prefix
    dec.reset()
    before = dec.prefix_stats()
    got = dec.generate_batch([[9, 8, 7], p, p], [0, 10, 10], lanes=2, lane_context=64)
    assert got == [[], e, e]
    assert _delta(dec, before) == (2 * (len(p) - 1), len(p) - 1 + 2)
    # prompts that share nothing: every prompt is computed whole, nothing is copied
    q = [[5, 6, 7], [8, 9]]
    before = dec.prefix_stats()
    dec.generate_batch(q, 2, lanes=2, lane_context=64)
    assert _delta(dec, before) == (0, 5)


# ---- 7. Chat and Generator -------------------------------------------------------------------------------------------------------

def test_chat_turn_two_reuses_turn_one(tmp_path):
    from kjarni_amd.chat import Chat, GenerationConfig
    d = str(tmp_path / "chat")
    cfg, t = synth.llm_model(d, synth.LLAMA_TEST, seed=11, vocab_size=720, bos_token_id=700, eos_token_id=[701, 705, 704])
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    greedy = GenerationConfig(do_sample=False, max_new_tokens=10)
    m1, m2 = "My name is Xylophone7492.", "What is my name?"
    plain = Chat("llama3.2-1b-instruct", model_path=d)
    convo = plain.conversation()
    want = [convo.send(m1, greedy), convo.send(m2, greedy)]
    assert plain.prefix_stats() == (0, 0)
    ids1 = plain.encode(plain.format_prompt([("user", m1)], None))
    ids2 = plain.encode(plain.format_prompt([("user", m1), ("assistant", want[0]), ("user", m2)], None))
    assert _lcp(ids1, ids2) == len(ids1), "precondition: turn 2's prompt begins with turn 1's"
    orc = L.LlmOracle(t, cfg)
    _, gap = LC.oracle_runs(orc, [ids1, ids2], 10)
    assert gap >= LC.GAP, f"precondition: {gap:.2e}"
    chat = Chat("llama3.2-1b-instruct", model_path=d)
    chat.set_prefix_reuse(True)
    convo = chat.conversation()
    assert convo.send(m1, greedy) == want[0]
    assert chat.prefix_stats() == (0, len(ids1))
    assert convo.send(m2, greedy) == want[1]
    reused, computed = chat.prefix_stats()
    assert reused >= len(ids1) - 1 and reused + computed == len(ids1) + len(ids2)
    print(f"chat: turn 2 kept {reused} of {len(ids2)} prompt tokens")


CONTEXT = "The quick brown fox jumps over the lazy dog. Once upon a time there was a small"
CONTINUATIONS = [" fox in a hole", " dog", " time in the ground there lived"]


def test_generator_score_reuses_the_context(tmp_path):
    from kjarni_amd import Generator
    d = str(tmp_path / "gpt2")
    cfg, t = G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    ref = S.Gpt264(t, cfg)
    gen = Generator("gpt2", model_path=d)
    first = len(gen.encode(CONTEXT))
    wholes = [gen.encode(CONTEXT + c) for c in CONTINUATIONS]
    assert all(_lcp(w, wholes[0]) >= first - 1 for w in wholes), "precondition: the continuations leave the context's tokens alone"
    off = [gen.score(CONTEXT, c) for c in CONTINUATIONS]
    assert gen.prefix_stats() == (0, 0)
    gen.set_prefix_reuse(True)
    prev = wholes[-1]                                       # (what the last reuse-off call left)
    for c, w, o in zip(CONTINUATIONS, wholes, off):
        before = gen.prefix_stats()
        total, n_tokens, is_greedy = gen.score(CONTEXT, c)
        keep = min(_lcp(prev, w), first - 1)
        assert keep >= first - 1 >= 1
        r, k = gen.prefix_stats()
        assert (r - before[0], k - before[1]) == (keep, len(w) - keep), c
        lg = ref.logits(w, ref.new())[first - 1:len(w) - 1]
        mx = lg.max(axis=1, keepdims=True)
        lsm = lg - (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))
        want = float(lsm[np.arange(len(w) - first), np.asarray(w[first:])].sum())
        assert n_tokens == len(w) - first == o[1]
        assert abs(total - want) <= n_tokens * 2.0 * _bar(lg), (c, total, want)
        prev = w
