"""Qwen3-MoE on the GPU: the router pick alone, the sparse FFN alone on both routes (the steps kernels, the grouped matrix-core
kernels) and whole models through the decoder's loops, against the float64 reference of tests/moe_ref64.py.

Bars: the ops alone 1e-5 * max(1, max |ref|); whole models llm_ref64.TOL (1e-4) * max(1, max |ref|).  Routing is discontinuous,
so experts and token ids are compared on inputs whose choice is clear: built with separated logits (the ops), or on the seeds
of tests/moe_fixture.py with the margins of moe_ref64.router_margins / qwen3_ref64.assert_margins asserted again here.  Inputs
carry NaN wherever a kernel must not read, outputs a guard band wherever it must not write.  The one-hot probes use small
integers (gate weights large enough that silu(g) == g in f32, tied pairs of experts so that the renormalised weights are exactly
0.5), so every product says which expert, row and column it came from, bit for bit."""
import os
import shutil

import numpy as np
import pytest

from tests import llm_ref64 as R
from tests import moe_fixture as F
from tests import qwen3_fixture as Q3
from tests.moe_ref64 import MoeRef64, moe_ffn64, route64, router_margins
from tests.qwen3_ref64 import assert_margins, log_softmax

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
F64 = np.float64
OP_TOL = 1e-5


def _within(got, ref, what, tol=R.TOL):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), tol * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def _bf16_exact(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _bits(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


# ---- 1. the route alone --------------------------------------------------------------------------------------------------------------

def _separated_logits(rng, rows, E):
    """Every row a permutation of E distinct values, shifted per row: the 12 largest 0.5 apart, the others 0.02 apart below them
    (max |logit| stays under 13, so 100 bars are at most 0.13)."""
    i = np.arange(E)
    base = np.where(i < 12, -0.5 * i, -6.0 - 0.02 * (i - 12))
    return np.stack([rng.permutation(base) + rng.uniform(-1, 1) for _ in range(rows)]).astype(np.float32)


@pytest.mark.parametrize("E,k", [(E, k) for E in (2, 8, 60, 128, 256) for k in (1, 2, 8) if k <= E])
def test_route_against_float64(E, k):
    from kjarni_amd import ops
    rng = np.random.default_rng(E * 10 + k)
    for rows in (1, 8, 300):
        logits = _separated_logits(rng, rows, E)
        order_clear = router_margins(logits, k, f"E {E} k {k} rows {rows}")
        assert order_clear.all()
        for norm in (False, True):
            ids, w = ops.moe_route(logits, k, norm)
            want_ids, want_w = route64(logits, k, norm)
            assert np.array_equal(ids, want_ids), (E, k, rows, norm)
            _within(w, want_w, f"E {E} k {k} rows {rows} norm {norm}", OP_TOL)
            if norm:
                assert np.abs(w.astype(F64).sum(-1) - 1.0).max() <= 1e-6


def test_route_ties_extremes_and_equal_logits():
    from kjarni_amd import ops
    r = np.full((6, 130), -3.0, np.float32)
    r[0, [5, 70, 129]] = 2.0                      # three equal maxima, in three different lane slots: 5, 70, 129 in that order
    r[1, [129, 64, 0]] = [1.0, 1.0, 1.5]          # 0 first, then the tie 64 before 129
    r[2, :] = 0.25                                # all equal: 0, 1, 2
    r[3, :] = -60.0
    r[3, [7, 100]] = 60.0                         # +-60: the losers' probabilities underflow in f32; the tie 7 before 100, then 0
    r[4, :] = np.linspace(-60, 60, 130)           # the largest last
    r[5, [3, 4]] = [0.0, -0.0]                    # -0 == +0: the lower index
    r[5, 5:] = -5.0
    r[5, :3] = -5.0
    ids, w = ops.moe_route(r, 3, False)
    want_ids, want_w = route64(r, 3, False)
    assert ids.tolist() == [[5, 70, 129], [0, 64, 129], [0, 1, 2], [7, 100, 0], [129, 128, 127], [3, 4, 0]]
    assert np.array_equal(ids, want_ids)
    _within(w, want_w, "ties", OP_TOL)
    assert w[0, 0] == w[0, 1] == w[0, 2] and w[3, 0] == w[3, 1] == 0.5 and w[3, 2] == 0.0
    ids, w = ops.moe_route(r, 3, True)
    _within(w, route64(r, 3, True)[1], "ties, renormalised", OP_TOL)
    assert np.array_equal(w[2], np.full(3, np.float32(1.0) / np.float32(3.0)))
    ids2, w2 = ops.moe_route(r, 3, True)
    assert np.array_equal(ids, ids2) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))


# ---- 2. the FFN alone ------------------------------------------------------------------------------------------------------------------

SEL = 16     # the first SEL columns of x select the row's group; the router reads nothing else


def _stacks(rng, H, Im, E, bf16):
    std = 1.0 / np.sqrt(H)
    gate = (rng.standard_normal((E, Im, H), dtype=np.float32) * np.float32(std * 2))
    up = (rng.standard_normal((E, Im, H), dtype=np.float32) * np.float32(std * 2))
    down = (rng.standard_normal((E, H, Im), dtype=np.float32) * np.float32(2.0 / np.sqrt(Im)))
    for e in range(E):     # experts of different sizes: the wrong expert is a large error
        down[e] *= np.float32(1.0 + e / E)
    return (_bf16_exact(gate), _bf16_exact(up), _bf16_exact(down)) if bf16 else (gate, up, down)


def _ffn_case(rng, rows, H, Im, E, k, groups, bf16, gamma=False, ldx=None, stacks=None):
    """groups: a list of (number of rows, experts in slot order) -- the rows of a group carry 4.0 in selector column g, and
    router[e, g] holds logits 0.5 apart for the chosen experts (largest first) and far below for the others, so the choice is
    clear by construction (asserted).  Rows are shuffled.  Returns a dict of everything the call and the reference need."""
    assert len(groups) <= SEL and sum(n for n, _ in groups) == rows
    x = rng.standard_normal((rows, H)).astype(np.float32)
    x[:, :SEL] = 0.0
    router = np.zeros((E, H), np.float32)
    owner = rng.permutation(np.repeat(np.arange(len(groups)), [n for n, _ in groups]))
    for g, (_, experts) in enumerate(groups):
        assert len(experts) == k
        router[:, g] = -2.0
        for j, e in enumerate(experts):
            router[e, g] = 1.0 - 0.125 * j
    x[np.arange(rows), owner] = 4.0
    gate, up, down = stacks or _stacks(rng, H, Im, E, bf16)
    gm = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32) if gamma else None
    if gamma:      # the norm rescales a row by 1 / rms: keep the selector dominant whatever the row
        gm[:SEL] = 1.0
    ld = ldx or H
    xp = np.full((rows, ld), np.nan, np.float32)
    xp[:, :H] = x
    xn = x.astype(F64)
    if gamma:
        xn = xn / np.sqrt((xn * xn).mean(-1, keepdims=True) + 1e-6) * gm.astype(F64)
    contrib, logits, ids, w = moe_ffn64(xn, router, gate, up, down, k, True)
    assert router_margins(logits, k, "case").all()
    assert all(ids[r].tolist() == list(groups[owner[r]][1]) for r in range(rows))
    return dict(x=xp, router=router, gate=gate, up=up, down=down, gamma=gm, contrib=contrib, ids=ids, w=w, owner=owner, rows=rows, H=H, k=k,
                bf16=bf16)


def _run_ffn(c, route, in_place, ldy=None):
    from kjarni_amd import ops
    rows, H = c["rows"], c["H"]
    rng = np.random.default_rng(99)
    res = rng.standard_normal((rows, H)).astype(np.float32)
    ld = ldy or H + 4
    y = np.full((rows, ld), np.nan, np.float32)          # the guard band behind every output row: NaN in, the same NaN out
    if in_place:
        y[:, :H] = res
    conv = _bits if c["bf16"] else (lambda a: a)
    got, ids, w, used, tiles = ops.moe_ffn(c["x"], conv(c["router"]), conv(c["gate"]), conv(c["up"]), conv(c["down"]), c["k"], y,
                                           r=None if in_place else np.concatenate([res, np.full((rows, 4), np.nan, np.float32)], axis=1),
                                           r_is_y=in_place, gamma=c["gamma"], eps=1e-6, norm_topk=True, bf16=c["bf16"], route=route)
    assert np.isnan(got[:, H:]).all(), "the guard band was written"
    return got[:, :H], res.astype(F64) + c["contrib"], ids, w, used, tiles


STEP_GEOMETRIES = [(64, 32, 8, 2), (512, 96, 16, 4), (64, 32, 128, 8), (2048, 768, 8, 8)]     # hidden, Im, E, k


def _step_groups(rows, E, k, kind):
    if kind == "same":
        return [(rows, [(1 + j) % E for j in range(k)])]
    if kind == "last":       # expert E - 1 first: the last stride of the stacks
        return [(rows, [E - 1] + list(range(k - 1)))]
    per = [[(r * k + j) % E for j in range(k)] for r in range(rows)]      # disjoint while rows * k <= E, then wrapping
    return [(1, p) for p in per]


@pytest.mark.parametrize("H,Im,E,k", STEP_GEOMETRIES)
@pytest.mark.parametrize("bf16", [False, True])
def test_ffn_steps_against_float64(H, Im, E, k, bf16):
    rng = np.random.default_rng(H + E + k + int(bf16))
    stacks = _stacks(rng, H, Im, E, bf16)          # one set of experts, four routings
    for rows, kind, in_place, gamma in ((1, "last", True, True), (2, "disjoint", False, False), (8, "same", True, False),
                                        (8, "disjoint", False, True)):
        c = _ffn_case(rng, rows, H, Im, E, k, _step_groups(rows, E, k, kind), bf16, gamma=gamma, ldx=H + 8, stacks=stacks)
        got, want, ids, w, used, tiles = _run_ffn(c, 1, in_place)
        assert (used, tiles) == (1, 0)
        assert np.array_equal(ids, c["ids"]), (rows, kind)
        _within(w, c["w"], f"{rows} rows {kind}: weights", OP_TOL)
        _within(got, want, f"{H}x{Im} E {E} k {k} bf16 {bf16}: {rows} rows {kind}", OP_TOL)


def _probe(rng, rows, H, Im, E, pairs_of_row):
    """Integer probe: x one-hot (column c_r), router[e, c] = 1 for the two experts of the rows that use column c (a tie: the
    lower index first, weights exactly 0.5), gate weights 20 .. 27 (silu(g) == g in f32), up / down small integers."""
    x = np.zeros((rows, H), np.float32)
    router = np.full((E, H), -4.0, np.float32)
    cols = rng.permutation(H)[:E * (E - 1) // 2]          # a column per distinct pair
    col_of = {}
    for r, pair in enumerate(pairs_of_row):
        key = tuple(sorted(pair))
        if key not in col_of:
            col_of[key] = cols[len(col_of)]
            router[list(key), col_of[key]] = 1.0
        x[r, col_of[key]] = 1.0
    gate = rng.integers(20, 28, (E, Im, H)).astype(np.float32)
    up = rng.integers(-3, 4, (E, Im, H)).astype(np.float32)
    down = rng.integers(-2, 3, (E, H, Im)).astype(np.float32)
    res = rng.integers(-8, 9, (rows, H)).astype(np.float32)
    want = res.astype(F64)
    for r, pair in enumerate(pairs_of_row):
        c = int(np.argmax(x[r]))
        for e in sorted(pair):
            want[r] += 0.5 * (down[e].astype(F64) @ (gate[e][:, c].astype(F64) * up[e][:, c]))
    ids = np.array([sorted(p) for p in pairs_of_row], np.int32)
    return x, router, gate, up, down, res, want, ids


@pytest.mark.parametrize("route,rows", [(1, 8), (1, 3), (2, 24), (2, 65), (2, 130)])
@pytest.mark.parametrize("bf16", [False, True])
def test_ffn_one_hot_probes_bit_for_bit(route, rows, bf16):
    from kjarni_amd import ops
    H, Im, E = 64, 32, 8
    rng = np.random.default_rng(rows * 3 + route)
    pairs = [tuple(rng.choice(E, 2, replace=False).tolist()) for _ in range(rows)]
    pairs[0] = (E - 1, 0)
    x, router, gate, up, down, res, want, want_ids = _probe(rng, rows, H, Im, E, pairs)
    conv = _bits if bf16 else (lambda a: a)
    y = np.full((rows, H + 4), np.nan, np.float32)
    y[:, :H] = res
    got, ids, w, used, tiles = ops.moe_ffn(x, conv(router), conv(gate), conv(up), conv(down), 2, y, r_is_y=True, norm_topk=True, bf16=bf16,
                                           route=route)
    assert used == route and np.array_equal(ids, want_ids) and (w == 0.5).all()
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(got[:, :H].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.isnan(got[:, H:]).all()


def _tiles_numpy(ids, E):
    counts = np.bincount(np.asarray(ids).reshape(-1), minlength=E)
    return int(((counts + 63) // 64).sum())


GROUPED_CASES = {
    # rows: groups of (rows, experts).  300: an expert with no row (6, 7), with exactly 64 slots (0, 1), with 65 (2, 3), with 171 (4, 5)
    24: [(10, [0, 1]), (9, [7, 2]), (5, [3, 0])],
    64: [(64, [5, 6])],                                      # every row on one pair of experts: one full tile each
    65: [(65, [7, 0])],                                      # one more: a second tile of one slot
    300: [(64, [0, 1]), (65, [2, 3]), (171, [4, 5])],
}


@pytest.mark.parametrize("rows", sorted(GROUPED_CASES))
@pytest.mark.parametrize("bf16", [False, True])
def test_ffn_grouped_against_float64(rows, bf16):
    H, Im, E, k = (512, 96, 16, 2) if rows == 24 else (64, 32, 8, 2)
    rng = np.random.default_rng(rows + int(bf16))
    c = _ffn_case(rng, rows, H, Im, E, k, GROUPED_CASES[rows], bf16, gamma=rows in (24, 300), ldx=H + (8 if rows == 65 else 0))
    got, want, ids, w, used, tiles = _run_ffn(c, 2, in_place=rows != 64)
    assert used == 2 and tiles == _tiles_numpy(c["ids"], E), (tiles, _tiles_numpy(c["ids"], E))
    if rows == 300:
        assert tiles == 1 + 1 + 2 + 2 + 3 + 3
    assert np.array_equal(ids, c["ids"])
    _within(w, c["w"], f"grouped {rows}: weights", OP_TOL)
    _within(got, want, f"grouped {rows} rows bf16 {bf16}", OP_TOL)
    again = _run_ffn(c, 2, in_place=rows != 64)[0]
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "the same call twice"


def test_ffn_grouped_wide_k():
    """k = 4 of 16 at the MOE_WIDE widths, 65 rows over three groups, Im no multiple of 64."""
    rng = np.random.default_rng(5)
    c = _ffn_case(rng, 65, 512, 96, 16, 4, [(30, [15, 0, 7, 3]), (34, [1, 2, 15, 4]), (1, [8, 9, 10, 11])], True, gamma=True)
    got, want, ids, w, used, tiles = _run_ffn(c, 0, in_place=True)      # the decoders' rule: 65 rows are grouped
    assert used == 2 and tiles == _tiles_numpy(c["ids"], 16) and np.array_equal(ids, c["ids"])
    _within(got, want, "grouped, k = 4", OP_TOL)


@pytest.mark.parametrize("bf16", [False, True])
def test_the_two_routes_agree_on_eight_rows(bf16):
    rng = np.random.default_rng(8)
    c = _ffn_case(rng, 8, 512, 96, 16, 4, _step_groups(8, 16, 4, "disjoint"), bf16, gamma=True)
    a, want, ids_a, w_a, used_a, _ = _run_ffn(c, 1, True)
    b, _, ids_b, w_b, used_b, tiles = _run_ffn(c, 2, True)
    auto = _run_ffn(c, 0, True)
    assert (used_a, used_b, auto[4]) == (1, 2, 1) and tiles == _tiles_numpy(c["ids"], 16)
    assert np.array_equal(ids_a, ids_b) and np.array_equal(auto[0].view(np.uint32), a.view(np.uint32))
    _within(w_a, w_b, "weights, route against route", OP_TOL)
    _within(a, b, "steps against grouped", OP_TOL)
    _within(b, want, "grouped against float64", OP_TOL)


# ---- 3. whole models -------------------------------------------------------------------------------------------------------------------

def _load(tmp, name, bf16=False, **over):
    import kjarni_amd
    geo = F.GEOMETRIES[name]
    d = str(tmp / f"{name}-{int(bf16)}")
    cfg, t = F.moe_model(d, geo, store_bf16=bf16, **over)
    dec = kjarni_amd.HipDecoder(d)
    assert dec.bf16 == bf16 and dec.hidden == cfg["hidden_size"]
    return dec, MoeRef64(t, cfg), cfg, t, d


def _check_cache(dec, cache, what):
    assert dec.cache_len() == cache[0][0].shape[0], what
    got = [dec.kv_rows(i) for i in range(len(cache))]
    for (layer, name), (err, bar) in sorted(R.cache_errors(got, cache).items()):
        assert err <= bar, f"{what}: layer {layer} {name}: {err:.3e} > {bar:.3e}"


def _check_routing(dec, ref, call, what):
    """The record of every sparse layer against the reference's `call`-th forward: the chosen sets exactly, the slot order where
    the reference's order is clear, the weights per expert to the bar."""
    for layer, calls in ref.routing.items():
        r, want_ids, want_w = calls[call]
        order_clear = router_margins(r, ref.k, f"{what}: layer {layer}")
        ids, w = dec.moe_routing(layer)
        assert ids.shape == want_ids.shape, (what, layer, ids.shape)
        assert np.array_equal(np.sort(ids, axis=-1), np.sort(want_ids, axis=-1)), f"{what}: layer {layer}: other experts"
        assert np.array_equal(ids[order_clear], want_ids[order_clear]), f"{what}: layer {layer}: slot order"
        by = np.argsort(ids, axis=-1)
        want_by = np.argsort(want_ids, axis=-1)
        _within(np.take_along_axis(w, by, -1), np.take_along_axis(want_w, want_by, -1), f"{what}: layer {layer} weights")


@pytest.mark.parametrize("name", sorted(F.GEOMETRIES))
@pytest.mark.parametrize("bf16", [False, True])
def test_model_against_float64(tmp_path, name, bf16):
    dec, ref, cfg, t, _ = _load(tmp_path, name, bf16)
    V = cfg["vocab_size"]
    # the steps route: a 9-token prompt is an 8-row pass and a 1-row pass; then 12 greedy tokens through the captured step
    prompt = F.seeded_prompt(F.GREEDY_PROMPT_SEED[(name, bf16)], V, 9)
    want, gaps, tops = ref.greedy(prompt, 12)
    assert_margins(gaps, tops, name)
    ref.assert_router_margins(name)
    assert cfg["eos_token_id"] not in want
    hidden, logits = dec.forward(prompt)
    again = MoeRef64(t, cfg)
    cache = again.new_cache()
    h = again.forward(prompt[:8], cache)
    h = again.forward(prompt[8:], cache)
    _within(logits, again.logits(h[-1:])[0], f"{name}: 9-token prompt logits")
    _within(hidden, again.final_norm(h[-1:]), f"{name}: hidden")
    _check_cache(dec, cache, f"{name} steps")
    _check_routing(dec, again, 1, f"{name}: the 1-row pass")
    dec.reset()
    dec.forward(prompt[:8])
    _check_routing(dec, again, 0, f"{name}: the 8-row pass")
    dec.reset()
    got = dec.generate(prompt, 12)
    assert got == want
    dec.reset()
    assert dec.generate(prompt, 12) == got, "a captured run twice"
    # the rows route: a 40-token prompt
    long = F.seeded_prompt(F.LONG_PROMPT_SEED[(name, bf16)], V, 40)
    rows_ref = MoeRef64(t, cfg)
    cache = rows_ref.new_cache()
    h = rows_ref.forward(long, cache)
    dec.reset()
    hidden, logits = dec.forward(long)
    _within(logits, rows_ref.logits(h[-1:])[0], f"{name}: 40-token prompt logits")
    _within(hidden, rows_ref.final_norm(h[-8:]), f"{name}: 40-token hidden rows")
    _check_cache(dec, cache, f"{name} rows")
    _check_routing(dec, rows_ref, 0, f"{name}: the 40-row pass")
    by = dec.weight_bytes_by_type()
    n_sparse = len(rows_ref.routing)
    stack = 3 * cfg["num_experts"] * cfg["moe_intermediate_size"] * cfg["hidden_size"] * (2 if bf16 else 4)
    assert sum(by.values()) >= n_sparse * stack


def test_mixed_dense_layer_is_the_qwen3_layer_bit_for_bit(tmp_path):
    """MOE_MIXED's layer 0 is dense: its K / V rows (which only layer 0's own weights and the embedding reach) are, bit for
    bit, those of the same tensors loaded as plain qwen3 with one layer."""
    import kjarni_amd
    dec, ref, cfg, t, _ = _load(tmp_path, "MOE_MIXED")
    dense_cfg = {k: v for k, v in cfg.items() if not k.startswith(("num_experts", "moe_", "norm_topk", "decoder_sparse", "mlp_only"))}
    dense_cfg.update(model_type="qwen3", num_hidden_layers=1)
    dense_t = {k: v for k, v in t.items() if not k.startswith("model.layers.1.")}
    plain = kjarni_amd.HipDecoder(Q3.write_dir(str(tmp_path / "plain"), dense_cfg, dense_t))
    ids = F.seeded_prompt(3, cfg["vocab_size"], 40)
    for block in (ids, ids[:5], ids[5:6]):
        dec.reset()
        plain.reset()
        dec.forward(block, fetch=False)
        plain.forward(block, fetch=False)
        (k0, v0), (k1, v1) = dec.kv_rows(0), plain.kv_rows(0)
        assert np.array_equal(k0.view(np.uint32), k1.view(np.uint32)) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32))
    # the dense layer's FFN as well: the same checkpoint cut to its dense layer, as qwen3_moe and as qwen3 -- hidden rows and logits
    one_cfg = dict(cfg, num_hidden_layers=1)
    one = kjarni_amd.HipDecoder(Q3.write_dir(str(tmp_path / "one"), one_cfg, dense_t))
    for block in (ids, ids[:5], ids[5:6]):
        one.reset()
        plain.reset()
        ha, la = one.forward(block)
        hb, lb = plain.forward(block)
        assert np.array_equal(ha.view(np.uint32), hb.view(np.uint32)) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    from kjarni_amd._ffi import KjarniException
    with pytest.raises(KjarniException) as e:
        one.moe_routing(0)
    assert "dense layer" in str(e.value)
    with pytest.raises(KjarniException) as e:
        dec.moe_routing(0)
    assert "dense layer" in str(e.value)
    with pytest.raises(KjarniException) as e:
        plain.moe_routing(0)
    assert "dense" in str(e.value)
    assert dec.moe_routing(1)[0].shape == (1, 2)


# ---- 4. the loops, against plain generate, on MOE_WIDE -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return _load(tmp_path_factory.mktemp("moe_wide"), "MOE_WIDE")


def _clear_greedy(t, cfg, prompt, n, what):
    ref = MoeRef64(t, cfg)
    want, gaps, tops = ref.greedy(prompt, n)
    assert_margins(gaps, tops, what)
    ref.assert_router_margins(what)
    assert cfg["eos_token_id"] not in want
    return want


def test_loops_equal_plain_generate(wide):
    dec, _, cfg, t, _ = wide
    import kjarni_amd.constraints as K
    V = cfg["vocab_size"]
    prompt = F.seeded_prompt(F.GREEDY_PROMPT_SEED[("MOE_WIDE", False)], V, 9)
    want = _clear_greedy(t, cfg, prompt, 12, "wide")
    dec.reset()
    assert dec.generate(prompt, 12) == want
    # a constraint that masks nothing: every token one byte the pattern allows
    con = K.Constraint(r"a*", [b"a"] * V)
    got, res = dec.generate_constrained(con, prompt, 12)
    assert got == want and not res["violated"]
    # sampled with fixed draws: the same ids twice, and greedy when the draws cannot matter (top_k = 1)
    a, _ = dec.generate_sampled(prompt, 12, temperature=0.8, top_k=1, seed=7)
    assert a == want
    b, _ = dec.generate_sampled(prompt, 12, temperature=0.8, top_k=20, seed=7)
    c, _ = dec.generate_sampled(prompt, 12, temperature=0.8, top_k=20, seed=7)
    assert b == c and len(b) == 12
    # prompt-lookup on a repeating prompt (verify blocks run the steps kernels with n = rows): the plain loop's ids
    rep_prompt = Q3.lookup_prompt(F.LOOKUP_PROMPT_SEED, V)
    rep_want = _clear_greedy(t, cfg, rep_prompt, 12, "lookup")
    dec.reset()
    assert dec.generate(rep_prompt, 12) == rep_want
    got, stats = dec.generate_lookup(rep_prompt, 12)
    assert got == rep_want and stats["verify_steps"] > 0
    # prefix reuse across two calls
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        assert dec.generate(prompt, 12) == want
        before = dec.prefix_stats()
        assert dec.generate(prompt, 12) == want
        reused = dec.prefix_stats()[0] - before[0]
        assert reused >= len(prompt) - 1
    finally:
        dec.set_prefix_reuse(False)
    s, f = dec.verify_gemv_calls()
    assert s > 0       # hidden 512: the verify blocks' projections stream


def test_lanes_and_draft_equal_plain_generate(wide, tmp_path):
    import kjarni_amd
    dec, _, cfg, t, _ = wide
    V = cfg["vocab_size"]
    prompts = [F.seeded_prompt(seed, V, n) for n, seed in F.LANE_PROMPTS]          # ragged
    want = [_clear_greedy(t, cfg, p, 8, f"lane prompt of {len(p)}") for p in prompts]
    dec.reset()
    assert [dec.generate(p, 8) for p in prompts] == want
    assert dec.generate_batch(prompts, 8, lanes=3, lane_context=64) == want
    # a dense Qwen3 drafter of the same vocabulary
    draft_dir = str(tmp_path / "drafter")
    Q3.qwen3_model(draft_dir, Q3.Q3_D128, seed=1)
    drafter = kjarni_amd.HipDecoder(draft_dir)
    got, stats = dec.generate_draft(drafter, prompts[1], 8, 4)
    assert got == want[1] and stats["verify_steps"] > 0


def test_score_and_packed_passes(wide):
    dec, _, cfg, t, _ = wide
    V = cfg["vocab_size"]
    ids = F.seeded_prompt(F.LONG_PROMPT_SEED[("MOE_WIDE", False)], V, 40)
    ref = MoeRef64(t, cfg)
    logits = ref.logits(ref.forward(ids, ref.new_cache()))[:-1]
    ref.assert_router_margins("score")
    lsm = log_softmax(logits)
    want = lsm[np.arange(39), ids[1:]]
    bar = 2.0 * R.TOL * max(1.0, float(np.abs(logits).max()))
    lp, top, tlp = dec.score(ids)
    assert np.isfinite(lp).all() and float(np.abs(lp.astype(F64) - want).max()) <= bar
    # score_batch against score() one by one (the packed pass routes the same rows through the grouped kernels)
    seqs = [ids, ids[:17], ids[:29]]          # prefixes of the clear prompt: causal, so their routing is the clear prompt's
    blp, bid, btlp = dec.score_batch(seqs, [1, 1, 1])
    one = np.concatenate([dec.score(s)[0] for s in seqs])
    assert float(np.abs(blp.astype(F64) - one).max()) <= bar


def test_embed_batch_against_float64(tmp_path):
    dec, _, cfg, t, _ = _load(tmp_path, "MOE_SMALL")
    V = cfg["vocab_size"]
    full = F.seeded_prompt(F.LONG_PROMPT_SEED[("MOE_SMALL", False)], V, 40)
    seqs = [full, full[:13], full[:29]]           # prefixes of the clear prompt: causal, so their routing is the clear prompt's
    ref = MoeRef64(t, cfg)
    h = ref.final_norm(ref.forward(full, ref.new_cache()))
    ref.assert_router_margins("embed")
    got = dec.embed(seqs, normalize=False)
    for i, s in enumerate(seqs):
        _within(got[i], h[len(s) - 1], f"embed sequence {i}")


# ---- 5. front ends ----------------------------------------------------------------------------------------------------------------------

def test_chat_and_generator_run_a_moe_directory(tmp_path):
    import kjarni_amd
    from kjarni_amd import Generator
    from kjarni_amd.chat import Chat, GenerationConfig
    d = str(tmp_path / "chat")
    cfg, t = F.moe_model(d, F.MOE_SMALL, vocab_size=720, bos_token_id=700, eos_token_id=702)
    shutil.copy(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    chat = Chat("Qwen/Qwen3-30B-A3B", model_path=d)
    assert chat.model_name == "qwen3-30b-a3b"
    prompt = chat.format_prompt(None, "Hi")
    assert prompt.startswith("<|im_start|>system\n")
    ids = chat.encode(prompt)
    dec = kjarni_amd.HipDecoder(d)
    want = dec.generate(ids, 6)
    del dec
    pieces = []
    chat.stream("Hi", pieces.append, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=6))
    assert len(pieces) == len(want) > 0
    del chat
    gen = Generator("qwen3-30b-a3b", model_path=d)
    assert gen.generate(prompt, GenerationConfig(do_sample=False, repetition_penalty=1.0, max_new_tokens=6)) == "".join(pieces)
