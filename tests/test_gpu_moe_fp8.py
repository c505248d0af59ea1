"""Qwen3-MoE over FP8 expert stacks on the GPU against float64 (tests/moe_ref64.py over dequantized weights): the kernels through the op
hook at 1e-5 * max(1, max |ref|), every call twice for the same bits; then a 2-layer FP8 checkpoint through the decoder's loops."""
import os
import shutil

import numpy as np
import pytest

from tests import fp8_fixture as Q
from tests import llm_ref64 as R
from tests import moe_fixture as F
from tests import test_moe_fp8_host as M     # (the fixture lives with the host tests)
from tests.moe_ref64 import MoeRef64, moe_ffn64, router_margins
from tests.qwen3_ref64 import assert_margins

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F64, OP_TOL, SEL = np.float64, 1e-5, 8

def _within(got, ref, what, tol=R.TOL):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), tol * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e} ({err / bar:.3f} of the bar)")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"

def _stack(rng, E, n, k, kind, std, spread):     # (codes, scales [E, extent], dequantized); spread: neighbouring block scales 2^6 apart
    codes, scales, deq = [], [], []
    for e in range(E):
        w = rng.standard_normal((n, k), dtype=np.float32) * np.float32(std * (1.0 + e / E))     # a wrong expert is a large error
        c, s = Q.quantize(w, kind, rng)
        if spread and kind == "block":
            s = (s * 64.0 ** (np.add.outer(np.arange(s.shape[0]), np.arange(s.shape[1])) % 2)).astype(np.float32)
            c = Q.encode(w.astype(F64) / Q.expand_scale(s, kind, n, k))
        codes.append(c), scales.append(s.reshape(-1)), deq.append(Q.dequantize(c, s, kind))
    return np.stack(codes), np.stack(scales), np.stack(deq)

def _case(seed, rows, H, Im, E, k, kind, groups, gamma=False, ldx=None, spread=True):
    """groups: (rows, experts in slot order); a selector column per group makes the choice clear by construction (asserted)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, H)).astype(np.float32)
    x[:, :SEL] = 0.0
    router = np.zeros((E, H), np.float32)
    owner = rng.permutation(np.repeat(np.arange(len(groups)), [n for n, _ in groups]))
    for g, (_, experts) in enumerate(groups):
        router[:, g] = -2.0
        router[list(experts), g] = 1.0 - 0.125 * np.arange(k)
    x[np.arange(rows), owner] = 4.0
    gate, up = (_stack(rng, E, Im, H, kind, 2.0 / np.sqrt(H), spread) for _ in range(2))
    down = _stack(rng, E, H, Im, kind, 2.0 / np.sqrt(Im), spread)
    xp = np.full((rows, ldx or H), np.nan, np.float32)
    xp[:, :H] = x
    gm, xn = None, x.astype(F64)
    if gamma:
        gm = np.concatenate([np.ones(SEL), 1.0 + 0.1 * rng.standard_normal(H - SEL)]).astype(np.float32)
        xn = xn / np.sqrt((xn * xn).mean(-1, keepdims=True) + 1e-6) * gm.astype(F64)
    contrib, logits, ids, w = moe_ffn64(xn, router, gate[2], up[2], down[2], k, True)
    assert router_margins(logits, k, "case").all()
    assert all(ids[r].tolist() == list(groups[owner[r]][1]) for r in range(rows))
    return dict(x=xp, router=router, gate=gate[:2], up=up[:2], down=down[:2], gamma=gm, contrib=contrib, ids=ids, w=w, rows=rows, H=H, k=k, kind=kind)

def _twice(y, H, *args, **kw):
    """ops.moe_ffn_fp8 twice for the same bits; NaN stays in the band behind every output row.  Returns (y[:, :H], ids, weights, tiles)."""
    from kjarni_amd import ops
    a, b = (ops.moe_ffn_fp8(*args, y=y, norm_topk=True, **kw) for _ in range(2))
    assert np.isnan(a[0][:, H:]).all(), "the band behind the output rows was written"
    assert all(np.array_equal(np.asarray(u).view(np.uint32), np.asarray(v).view(np.uint32)) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]
    return a[0][:, :H], a[1], a[2], a[3]

def _run(c, grouped, in_place):
    rows, H = c["rows"], c["H"]
    res = np.random.default_rng(99).standard_normal((rows, H)).astype(np.float32)
    y = np.full((rows, H + 4), np.nan, np.float32)
    if in_place:
        y[:, :H] = res
    r = None if in_place else np.concatenate([res, np.full((rows, 4), np.nan, np.float32)], axis=1)
    got, ids, w, tiles = _twice(y, H, c["x"], c["router"], c["gate"], c["up"], c["down"], c["kind"], c["k"], r=r, r_is_y=in_place, gamma=c["gamma"],
                                grouped=grouped)
    return got, res.astype(F64) + c["contrib"], ids, w, tiles

def _disjoint(rows, E, k):
    return [(1, [(r * k + j) % E for j in range(k)]) for r in range(rows)]

# (grouped, rows, (hidden, Im, E, k), groups, in place, gamma, ldx - hidden).  Steps: rows 1 / 3 / 8 per shape, Im 96 per channel only;
# grouped 130: experts with no row (6, 7), with exactly 64 slots (0, 1), with 65 (2, 3)
CASES = [(False, rows, s, [(rows, [s[2] - 1] + list(range(s[3] - 1)))] if rows == 1 else _disjoint(rows, s[2], s[3]), rows != 3, rows != 3, 8)
         for s in ((128, 128, 4, 1), (256, 384, 8, 2), (256, 96, 8, 2)) for rows in (1, 3, 8)] + [
    (True, 24, (256, 384, 8, 2), [(10, [0, 1]), (9, [7, 2]), (5, [3, 0])], False, True, 8), (True, 65, (128, 128, 4, 1), [(65, [3])], True, False, 0),
    (True, 130, (128, 128, 8, 2), [(64, [0, 1]), (65, [2, 3]), (1, [4, 5])], True, True, 0)]

@pytest.mark.parametrize("kind,case", [(kd, c) for kd in Q.KINDS for c in CASES if c[2][1] % 128 == 0 or kd == "channel"])
def test_both_routes_against_float64(kind, case):
    grouped, rows, (H, Im, E, k), groups, in_place, gamma, pad = case
    c = _case(H + Im + rows, rows, H, Im, E, k, kind, groups, gamma=gamma, ldx=H + pad)
    got, want, ids, w, tiles = _run(c, grouped, in_place)
    counts = np.bincount(c["ids"].reshape(-1), minlength=E)
    assert tiles == (int(((counts + 63) // 64).sum()) if grouped else 0) and np.array_equal(ids, c["ids"])
    assert rows != 130 or sorted(counts.tolist()) == [0, 0, 1, 1, 64, 64, 65, 65]
    _within(w, c["w"], f"{kind} {rows} rows: weights", OP_TOL)
    _within(got, want, f"{'grouped' if grouped else 'steps'} {kind} {H}x{Im} E {E} k {k}: {rows} rows", OP_TOL)

@pytest.mark.parametrize("kind", Q.KINDS)
def test_the_two_routes_agree_on_eight_rows(kind):
    c = _case(8, 8, 256, 384, 8, 2, kind, _disjoint(8, 8, 2), gamma=True)
    a, want, ids_a, w_a, _ = _run(c, False, True)
    b, _, ids_b, w_b, tiles = _run(c, True, True)
    assert np.array_equal(ids_a, ids_b) and tiles == 8
    _within(w_a, w_b, "weights, route against route", OP_TOL)
    _within(a, b, f"{kind}: steps against grouped", OP_TOL)
    _within(b, want, f"{kind}: grouped against float64", OP_TOL)

@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("grouped,rows", [(False, 8), (False, 3), (True, 24), (True, 65), (True, 130)])
def test_every_code_on_one_hot_rows_bit_for_bit(kind, grouped, rows):
    """x one-hot, two tied experts per row (weights 0.5), gate 20 / 24 / 28 (silu(g) == g in f32), all 254 codes in up: exact sums."""
    H, Im, E = 128, 128, 4
    rng = np.random.default_rng(rows + 7 * grouped)
    pairs = [tuple(sorted(rng.choice(E, 2, replace=False).tolist())) for _ in range(rows)]
    cols = dict(zip(sorted(set(pairs)), rng.permutation(H)))
    x, router = np.zeros((rows, H), np.float32), np.full((E, H), -4.0, np.float32)
    for r, p in enumerate(pairs):
        x[r, cols[p]] = 1.0
        router[list(p), cols[p]] = 1.0
    ones = lambda n, k: np.ones((E, int(np.prod(Q.scale_shape(kind, n, k)))), np.float32)  # noqa: E731
    gate = Q.encode(rng.choice([20.0, 24.0, 28.0], (E, Im, H)))
    up = np.resize(rng.permutation(Q.FINITE_CODES), (E, Im, H)).astype(np.uint8)
    down = np.zeros((E, H, Im), np.uint8)
    down[:, np.arange(H), np.arange(H) % Im] = Q.encode(rng.choice([-2.0, -1.0, 1.0, 2.0], (E, H)))
    gs = ones(Im, H) * rng.choice([1.0, 2.0], ones(Im, H).shape).astype(np.float32)
    deq = lambda c, sc: np.stack([Q.dequantize(c[e], sc[e], kind) for e in range(E)]).astype(F64)  # noqa: E731
    g64, u64, d64 = deq(gate, gs), deq(up, ones(Im, H)), deq(down, ones(H, Im))
    assert len(np.unique(up)) == 254
    res = rng.integers(-8, 9, (rows, H)).astype(np.float32)
    want = res.astype(F64)
    for r, p in enumerate(pairs):
        for e in p:
            want[r] += 0.5 * (d64[e] @ (g64[e][:, cols[p]] * u64[e][:, cols[p]]))
    assert (want.astype(np.float32).astype(F64) == want).all()
    y = np.full((rows, H + 4), np.nan, np.float32)
    y[:, :H] = res
    got, ids, w, _ = _twice(y, H, x, router, (gate, gs), (up, ones(Im, H)), (down, ones(H, Im)), kind, 2, r_is_y=True, grouped=grouped)
    assert np.array_equal(ids, np.array(pairs, np.int32)) and (w == 0.5).all()
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))

def _load(tmp, kind, **over):
    import kjarni_amd
    d = str(tmp / kind)
    cfg, hf = M.fp8_moe_model(d, kind, **over)
    H, Im = cfg["hidden_size"], cfg["moe_intermediate_size"]      # a [1, 1] scale would load as per tensor: the stacks must be of `kind`
    assert kind != "block" or (Q.scale_shape(kind, Im, H) == (2, 2) == Q.scale_shape(kind, H, Im))
    return kjarni_amd.HipDecoder(d), cfg, hf, d

def _clear_greedy(hf, cfg, prompt, n, what):
    ref = MoeRef64(hf, cfg)
    ids, gaps, tops = ref.greedy(prompt, n)
    assert_margins(gaps, tops, what)
    ref.assert_router_margins(what)
    return ids

def _check(dec, ref, cache, h, hidden, logits, call, what):
    ref.assert_router_margins(what)
    _within(logits, ref.logits(h[-1:])[0], f"{what}: logits")
    _within(hidden, ref.final_norm(h[-hidden.shape[0]:]), f"{what}: hidden")
    assert dec.cache_len() == cache[0][0].shape[0]
    for (layer, name), (err, bar) in sorted(R.cache_errors([dec.kv_rows(i) for i in range(len(cache))], cache).items()):
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e}"
    for layer, calls in ref.routing.items():
        r, want_ids, want_w = calls[call]
        clear = router_margins(r, ref.k, what)
        ids, w = dec.moe_routing(layer)
        assert np.array_equal(np.sort(ids, -1), np.sort(want_ids, -1)) and np.array_equal(ids[clear], want_ids[clear]), f"{what}: experts"
        _within(np.take_along_axis(w, np.argsort(ids, -1), -1), np.take_along_axis(want_w, np.argsort(want_ids, -1), -1), f"{what}: weights")

@pytest.mark.parametrize("kind", ["block", "channel"])
def test_model_and_wide_lanes_against_float64(tmp_path, kind):
    dec, cfg, hf, _ = _load(tmp_path, kind)
    V = cfg["vocab_size"]
    by = dec.weight_bytes_by_type()
    assert by["F8_E4M3"] >= 3 * cfg["num_experts"] * cfg["moe_intermediate_size"] * cfg["hidden_size"] and "BF16" not in by
    long = F.seeded_prompt(M.LONG_PROMPT_SEED[kind], V, 130)
    for n, mc in ((24, False), (130, False), (130, True)):     # the prompt route; its attention projections on the matrix cores too
        dec.set_fp8_matrix_cores(mc)
        dec.reset()
        ref = MoeRef64(hf, cfg)
        cache = ref.new_cache()
        h = ref.forward(long[:n], cache)
        hidden, logits = dec.forward(long[:n])
        _check(dec, ref, cache, h, hidden, logits, 0, f"{kind} {n} tokens mc {mc}")
    dec.set_fp8_matrix_cores(False)
    prompt = F.seeded_prompt(M.GREEDY_PROMPT_SEED[kind], V, 9)     # the steps route: an 8-row pass, a 1-row pass, the captured step
    want = _clear_greedy(hf, cfg, prompt, 12, kind)
    ref = MoeRef64(hf, cfg)
    cache = ref.new_cache()
    ref.forward(prompt[:8], cache)
    h = ref.forward(prompt[8:], cache)
    dec.reset()
    hidden, logits = dec.forward(prompt)
    _check(dec, ref, cache, h, hidden, logits, 1, f"{kind} 9-token prompt")
    for _ in range(2):
        dec.reset()
        assert dec.generate(prompt, 12) == want
    if kind == "block":     # 16 wide lanes: refused until the switch is on, then the reference's tokens; 8 lanes on the steps route
        prompts = [F.seeded_prompt(s, V, 3 + i) for i, s in enumerate(M.LANE_PROMPT_SEEDS)]
        want = [_clear_greedy(hf, cfg, p, 8, "lanes") for p in prompts]
        with pytest.raises(Exception, match="more than 8 lanes"):
            dec.generate_wide(prompts, 8, lanes=16)
        dec.set_fp8_matrix_cores(True)
        assert dec.generate_wide(prompts, 8, lanes=16) == want and dec.generate_batch(prompts[:8], 8) == want[:8]

def test_chat_and_generator_run_an_fp8_moe_directory(tmp_path):
    from kjarni_amd import Generator
    from kjarni_amd.chat import Chat, GenerationConfig
    dec, cfg, hf, d = _load(tmp_path, "block", vocab_size=720, bos_token_id=700, eos_token_id=702)
    shutil.copy(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    chat = Chat("Qwen/Qwen3-30B-A3B", model_path=d)
    prompt = chat.format_prompt(None, "Hi")
    want = dec.generate(chat.encode(prompt), 6)
    del dec
    pieces = []
    chat.stream("Hi", pieces.append, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=6))
    assert len(pieces) == len(want) > 0
    del chat
    gen = Generator("qwen3-30b-a3b", model_path=d)
    assert gen.generate(prompt, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=6)) == "".join(pieces)
