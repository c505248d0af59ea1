"""What every generation loop leaves behind, for every way a run can end.

The loops (generate: plain greedy / processors / sampled on the device / sampled on the host; generate_lookup;
generate_lookup_sampled; generate_lanes: fast and slow) share one bookkeeping rule -- a token joins the output unless the run is
at its limit or the token is a stop id -- and differ in whether the last token of a run is fed to another step.  That difference
shows in cache_len(), resident() and lane_cache_len(), and is pinned here:

  * the processor / sampling loops of generate() feed every token they emit except the one after which the callback cancels
    or that fills the context.  Their rule would feed the last token of a run that ends on max_new_tokens, but max_len
    -- prompt + max_new_tokens wherever the C API builds the options -- is met by that same token, so the run leaves
    prompt + max_new_tokens - 1 rows; only an explicit larger max_len (C++ callers) shows the difference, and that
    is asserted on the host (tests/test_generation_run_host.py);
  * plain greedy runs bursts of graph replays sized by what is left of max_new_tokens and of the cache, so it leaves
    prompt + max_new_tokens - 1 rows on a max_new_tokens end: the last token is not fed;
  * the sampled lookup loop leaves prompt + emitted - 1; the greedy lookup loop at least that (its device runs ahead);
  * a lane leaves prompt + emitted - 1, or prompt + emitted when a stop id ended the request (the token before it was fed).

resident() is always (prompt + emitted)[:cache_len()].  A sampled loop takes one draw per decided token (the emitted ones and a
sampled stop id), counted here by sampling_routes() where the loop counts (the host-side sampler does not) and, for every
sampled loop, by changing the draws behind the last one used: the ids stay.  With n_uniforms = max_new_tokens a draw too many is
refused by the API, and the ids agreeing across the loops says the draws were used in order.

max_len has no field in the C API (it is always prompt + max_new_tokens there), so a run that ends on it is a run that ends on
max_new_tokens; the rule for an explicit max_len is covered on the host (tests/test_generation_run_host.py)."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu
CAP = 20                      # max_context: a 12-token prompt with 10 new tokens ends at the capacity
SAMPLED = dict(temperature=0.7, top_k=40, top_p=0.9, min_p=0.05)
PENALTY = 1.3
LOOKUP = (7, 3, 1)
N_NEW = 8
CB_BURST = 4                  # plain greedy and the fast lanes replay this many steps between two looks when a callback listens
LOOPS = ("greedy", "penalty", "penalty-host", "sampled", "sampled-host", "lookup", "lookup-sampled")
# generate()'s processor / sampling loops: the host feeds every token it decides to one more step.  Their rule would feed the last
# token of max_new_tokens too (LastToken::Fed), which cannot be seen in these runs: max_len = prompt + max_new_tokens stops it.
STEP_PER_TOKEN = ("penalty", "penalty-host", "sampled", "sampled-host")
DRAWS = ("sampled", "sampled-host", "lookup-sampled")
COUNTED = ("penalty", "sampled", "lookup-sampled")                    # sampling_routes() counts the tokens these decide


def _model(tmp_path, name, seed, **over):
    import kjarni_amd
    d = str(tmp_path / name)
    synth.llm_model(d, synth.LLAMA_TEST, seed=seed, **over)
    return kjarni_amd.HipDecoder(d, max_context=CAP)


@pytest.fixture(scope="module")
def dec(tmp_path_factory):
    return _model(tmp_path_factory.mktemp("generation_state"), "m", 4)


def _prompt(seed, n):
    a = np.random.default_rng(seed).integers(4, synth.LLAMA_TEST["vocab_size"], 4).tolist()
    return (a * 5)[:n]        # repeats, so the lookup loops draft


def _uniforms(seed, n):
    return np.random.default_rng(seed).random(n).astype(np.float32)


def _run(dec, loop, prompt, max_new, uniforms=None, stop_ids=None, on_token=None):
    """One run of `loop`: (ids, cache_len, resident, tokens decided from candidates + from a logits row)."""
    dec.set_device_sampling(not loop.endswith("-host"))
    before = sum(dec.sampling_routes())
    if loop == "lookup":
        ids, _ = dec.generate_lookup(prompt, max_new, *LOOKUP, stop_ids=stop_ids, on_token=on_token)
    else:
        kw = dict(stop_ids=stop_ids, on_token=on_token, lookup=LOOKUP if loop == "lookup-sampled" else None)
        if loop in DRAWS:
            ids, _ = dec.generate_sampled(prompt, max_new, sample=True, uniforms=uniforms if max_new else None, **SAMPLED, **kw)
        else:
            ids, _ = dec.generate_sampled(prompt, max_new, sample=False, repetition_penalty=1.0 if loop == "greedy" else PENALTY, **kw)
    dec.set_device_sampling(True)
    return ids, dec.cache_len(), dec.resident(), sum(dec.sampling_routes()) - before


def _base(dec, loop, prompt, max_new, seed=11):
    u = _uniforms(seed, max_new)
    ids, cache_len, resident, decided = _run(dec, loop, prompt, max_new, u)
    assert len(ids) == max_new, f"precondition: {loop} met a stop id of the model"
    return u, ids, cache_len, resident, decided


def _check_common(loop, prompt, ids, cache_len, resident, decided, draws):
    assert resident == (list(prompt) + ids)[:cache_len], loop
    assert cache_len <= CAP, loop
    # the counters: one per token decided on the device's side of a processor / sampling loop, none elsewhere
    counted = draws if loop in COUNTED else 0
    assert decided == counted, (loop, decided, counted)


@pytest.mark.parametrize("loop", LOOPS)
def test_max_new_tokens_ends_the_run(dec, loop):
    prompt = _prompt(1, 7)
    u, ids, cache_len, resident, decided = _base(dec, loop, prompt, N_NEW)
    _check_common(loop, prompt, ids, cache_len, resident, decided, N_NEW)
    if loop in STEP_PER_TOKEN:
        # the processor / sampling loops would feed the last token of max_new_tokens, but it is also the token that meets
        # max_len = prompt + max_new_tokens, and the token that fills the context is never fed
        assert cache_len == len(prompt) + N_NEW - 1, loop
    elif loop == "greedy":
        assert cache_len == len(prompt) + N_NEW - 1             # plain greedy does not feed the last token: its burst is one short
    elif loop == "lookup-sampled":
        assert cache_len == len(prompt) + N_NEW - 1
    else:
        assert cache_len >= len(prompt) + N_NEW - 1
    # nothing to generate: the prompt is prefilled and stays
    ids0, cache0, resident0, decided0 = _run(dec, loop, prompt, 0)
    assert ids0 == [] and cache0 == len(prompt) and resident0 == prompt and decided0 == 0, loop


def test_ids_agree_across_the_loops(dec):
    prompt = _prompt(1, 7)
    got = {loop: _base(dec, loop, prompt, N_NEW)[1] for loop in LOOPS}
    assert got["sampled"] == got["sampled-host"] == got["lookup-sampled"]
    assert got["greedy"] == got["lookup"]
    assert got["penalty"] == got["penalty-host"]


@pytest.mark.parametrize("loop", LOOPS)
def test_a_stop_id_ends_the_run(dec, loop):
    found = None
    for seed in range(1, 9):                                    # the first seeded prompt whose run has a token to stop at
        prompt = _prompt(seed, 7)
        u, base, _, _, _ = _base(dec, loop, prompt, N_NEW)
        first = [i for i in range(1, N_NEW) if base[i] not in base[:i]]
        if first:
            found = first[-1]
            break
    assert found is not None, "precondition: every run repeats its first token"
    k = found
    ids, cache_len, resident, decided = _run(dec, loop, prompt, N_NEW, u, stop_ids=[base[k]])
    assert ids == base[:k], loop
    _check_common(loop, prompt, ids, cache_len, resident, decided, k + 1)     # the stop id was decided (and drawn) too
    if loop in STEP_PER_TOKEN:
        assert cache_len == len(prompt) + k                     # every emitted token was fed: the stop id came from the last one
    elif loop == "greedy":
        assert cache_len == len(prompt) + N_NEW - 1             # the burst ran on past the stop; its rows do not count as resident
    elif loop == "lookup-sampled":
        assert cache_len == len(prompt) + k - 1
    else:
        assert cache_len >= len(prompt) + k - 1
    if loop in DRAWS:
        u2 = u.copy()
        u2[k + 1:] = 0.999                                      # (draw k decided the stop id; nothing behind it is read)
        assert _run(dec, loop, prompt, N_NEW, u2, stop_ids=[base[k]])[0] == ids
    # a stop id as the first token: nothing is emitted, one token was decided
    ids, cache_len, resident, decided = _run(dec, loop, prompt, N_NEW, u, stop_ids=[base[0]])
    assert ids == [] and resident == prompt[:cache_len], loop
    assert decided == (1 if loop in COUNTED else 0), loop
    # (the sampled lookup loop leaves prompt + emitted - 1 here too: the last prompt token's row does not count)
    assert cache_len == len(prompt) - (1 if loop == "lookup-sampled" else 0), loop


@pytest.mark.parametrize("loop", LOOPS)
def test_the_capacity_ends_the_run(dec, loop):
    prompt = _prompt(2, 12)
    room = CAP - len(prompt)
    u = _uniforms(12, 10)
    ids, cache_len, resident, decided = _run(dec, loop, prompt, 10, u)
    assert len(ids) == room, loop
    _check_common(loop, prompt, ids, cache_len, resident, decided, room)      # no draw is taken for a token that cannot be emitted
    if loop == "greedy":
        assert cache_len == CAP                                 # the burst fills the cache: min(max_new - 1, capacity - prompt) steps
    elif loop == "lookup":
        assert CAP - 1 <= cache_len <= CAP
    else:
        assert cache_len == CAP - 1, loop                       # the token that filled the context is not fed
    if loop in DRAWS:                                           # `room` draws were taken: the ones behind them are never read
        u2 = u.copy()
        u2[room:] = 0.999
        assert _run(dec, loop, prompt, 10, u2)[0] == ids, loop
    # a prompt that fills the capacity: nothing is decided
    full = _prompt(3, CAP)
    ids, cache_len, resident, decided = _run(dec, loop, full, 4, _uniforms(13, 4))
    assert ids == [] and cache_len == CAP and resident == full and decided == 0, loop


@pytest.mark.parametrize("loop", LOOPS)
def test_the_callback_ends_the_run_at_token_2(dec, loop):
    prompt = _prompt(1, 7)
    u, base, _, _, _ = _base(dec, loop, prompt, N_NEW)
    seen = []
    ids, cache_len, resident, decided = _run(dec, loop, prompt, N_NEW, u, on_token=lambda t: seen.append(t) or len(seen) < 2)
    assert ids == seen == base[:2], loop
    if loop in DRAWS:                                           # two draws were taken: the ones behind them are never read
        u2, seen2 = u.copy(), []
        u2[2:] = 0.999
        assert _run(dec, loop, prompt, N_NEW, u2, on_token=lambda t: seen2.append(t) or len(seen2) < 2)[0] == ids, loop
    _check_common(loop, prompt, ids, cache_len, resident, decided, 2)
    if loop == "greedy":
        assert cache_len == len(prompt) + CB_BURST              # one burst of four steps behind the first token
    elif loop == "lookup":
        assert cache_len >= len(prompt) + 1
    else:
        assert cache_len == len(prompt) + 1, loop               # the token the callback refused to go on from is not fed


# ---- lanes: 2 lanes, 3 requests.  Request 0 wants one token, which its prefill decides, so its lane takes the next waiting
# request at once: on the fast path lane 0 is filled, and refilled, before lane 1 is looked at (it ends on request 1, lane 1 on
# request 2); the slow path starts both lanes first (lane 0 ends on request 2, lane 1 on request 1) -----------------------------

LANE_PROMPTS = [_prompt(21, 5), _prompt(22, 9), _prompt(23, 12)]
LANE_NEW = [1, 8, 6]
PATHS = {"fast": dict(), "slow": dict(repetition_penalty=PENALTY)}


def _single(dec, path, prompt, max_new):
    loop = "greedy" if path == "fast" else "penalty"
    ids = _run(dec, loop, prompt, max_new)[0]
    assert len(ids) == max_new, "precondition: met a stop id of the model"
    return ids


def _lanes(dec, path, max_new, prompts=LANE_PROMPTS, **kw):
    before = sum(dec.sampling_routes())
    got = dec.generate_batch(prompts, max_new, lanes=2, **PATHS[path], **kw)
    return got, [dec.lane_cache_len(0), dec.lane_cache_len(1)], sum(dec.sampling_routes()) - before


def _lens(path, rows1, rows2):
    """[lane 0, lane 1] when requests 1 and 2 leave rows1 and rows2 rows."""
    return [rows1, rows2] if path == "fast" else [rows2, rows1]


@pytest.mark.parametrize("path", list(PATHS))
def test_lanes_end_on_max_new_tokens_and_on_the_lane_capacity(dec, path):
    P, N = [len(p) for p in LANE_PROMPTS], LANE_NEW
    want = [_single(dec, path, p, m) for p, m in zip(LANE_PROMPTS, N)]
    got, lens, decided = _lanes(dec, path, N)
    assert got == want
    assert lens == _lens(path, P[1] + N[1] - 1, P[2] + N[2] - 1), path        # the last token of a request is not fed
    assert decided == (sum(N) if path == "slow" else 0)
    # a lane capacity of 14 rows: requests 1 and 2 end on it, after 5 and 2 tokens; the token that fills the lane is not fed
    got, lens, decided = _lanes(dec, path, N, lane_context=14)
    assert got == [want[0], want[1][:5], want[2][:2]]
    assert lens == [13, 13], path
    assert decided == (1 + 5 + 2 if path == "slow" else 0)
    # nothing to generate for request 1: it never enters a lane; lane 0 keeps request 0 (3 tokens), lane 1 takes request 2
    got, lens, _ = _lanes(dec, path, [3, 0, N[2]])
    assert got == [_single(dec, path, LANE_PROMPTS[0], 3), [], want[2]]
    assert lens == [P[0] + 3 - 1, P[2] + N[2] - 1], path


@pytest.mark.parametrize("path", list(PATHS))
def test_lanes_end_on_the_callback_at_token_2(dec, path):
    P, N = [len(p) for p in LANE_PROMPTS], LANE_NEW
    want = [_single(dec, path, p, m) for p, m in zip(LANE_PROMPTS, N)]
    seen = []

    def on_token(i, tok):
        seen.append((i, tok))
        return not (i == 2 and sum(1 for j, _ in seen if j == 2) == 2)
    got, lens, decided = _lanes(dec, path, N, on_token=on_token)
    assert got == [want[0], want[1], want[2][:2]]
    for i in range(3):
        assert [t for j, t in seen if j == i] == got[i]
    if path == "slow":   # the token the callback refused to go on from is not fed
        assert lens == _lens(path, P[1] + N[1] - 1, P[2] + 1)
        assert decided == N[0] + N[1] + 2
    else:                # the device went on to the end of the burst of four steps behind the first token
        assert lens == _lens(path, P[1] + N[1] - 1, P[2] + CB_BURST)


@pytest.mark.parametrize("path", list(PATHS))
def test_lanes_end_on_a_stop_id(dec, path, tmp_path):
    P, N = [len(p) for p in LANE_PROMPTS], LANE_NEW
    want = [_single(dec, path, p, m) for p, m in zip(LANE_PROMPTS, N)]
    # request 1 gets the seeded 9-token prompt whose run offers the latest token to stop at: one that first appears there and
    # that the other two requests never emit (index 0 when every run repeats its first token)
    best = None
    for seed in range(22, 38):
        base = _single(dec, path, _prompt(seed, P[1]), N[1])
        k = max(i for i in range(N[1]) if base[i] not in base[:i])
        if base[k] not in want[0] + want[2] and (best is None or k > best[0]):
            best = (k, seed, base)
    assert best is not None, "precondition: every candidate stop id is emitted by another request"
    k, seed, base = best
    prompts = [LANE_PROMPTS[0], _prompt(seed, P[1]), LANE_PROMPTS[2]]
    stopping = _model(tmp_path, "stop", 4, eos_token_id=[base[k]])              # the same weights; the observed token is the stop id
    got, lens, decided = _lanes(stopping, path, N, prompts=prompts)
    assert got == [want[0], base[:k], want[2]]
    # every emitted token of request 1 was fed: the stop id came from the last one
    assert lens == _lens(path, P[1] + k, P[2] + N[2] - 1), path
    assert decided == (N[0] + k + 1 + N[2] if path == "slow" else 0)
