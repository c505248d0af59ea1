"""Batched scoring on the GPU (kjarni_hip_decoder_score_batch, kjarni_hip_op_packed_prefix_attention,
kjarni_hip_op_score_gather_norm, kjarni_generator_score_batch).

The two kernels alone against numpy float64, with the rows and columns they must not touch; whole models -- independent
sequences and sequences that share a context -- against the float64 references with every row's logits; sharing against not
sharing; chunks; a prefix on the matrix-core route; the tile GEMM route; top-k; the state a call leaves; validation; the Generator.

Bars.  Logits carry the decoder's bar B = 1e-4 * max(1, max |ref logits|); lse is 1-Lipschitz in the sup norm, so logprob and
top_logprob get 2B against float64 and 4B where two device results are compared.  The arg-max is compared on every row: the
fixtures, seeds and batches below have no scored row whose two best float64 logits lie within lanes_cases.GAP (asserted).
Bit-for-bit comparisons are between two runs of the same arithmetic and say which existing kernel they follow."""
import ctypes as C

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import gpt2_fixture as G
from tests import lanes_cases as LC
from tests import qwen3_fixture as F
from tests import synth
from tests.test_gpu_lookup import _llama
from tests.test_gpu_score import _bar, _gaps, _last_max_rows, _log_softmax64, _model
from tests.test_gpu_score_topk import _check_topk, _same_bits

pytestmark = pytest.mark.gpu
F64 = np.float64
CANARY = np.float32(-777.25)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _within(got, ref, what, tol=1e-4):
    ref = np.asarray(ref, F64)
    err, bar = float(np.abs(np.asarray(got, F64) - ref).max()), tol * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


# ---- 1. prefix attention alone ---------------------------------------------------------------------------------------------------

PREFIX_SETS = [(1, [1, 1]), (31, [1, 32, 33]), (64, [5]), (65, [70, 3]), (200, [7, 40])]
ATT_CASES = [(d, g, ps) for d in (16, 32, 64, 128) for g in (1, 2, 4) for ps in PREFIX_SETS]


def _att_inputs(d, group, prefix, rems, seed):
    """Rows: 2 rows of another group, the prefix, the remainders one after another, 3 rows past the end."""
    kvh, heads = 2, 2 * group
    rng = np.random.default_rng(seed)
    T = 2 + prefix + sum(rems)
    rows = T + 3
    ldq, ldk, ldv, ldc = heads * d + 8, kvh * d + 4, kvh * d + 12, heads * d + 4
    q = rng.standard_normal((rows, ldq)).astype(np.float32)
    k = rng.standard_normal((rows, ldk)).astype(np.float32)
    v = rng.standard_normal((rows, ldv)).astype(np.float32)
    ctx = np.full((rows, ldc), CANARY, np.float32)
    table, at = [], 2 + prefix
    for n in rems:
        table.append((at, n, 2, prefix))
        at += n
    return heads, kvh, T, q, k, v, ctx, table


def _att_ref(q, k, v, first, n, pf, pl, heads, kvh, d):
    """float64 [n, heads * d]: the remainder's rows over the keys (prefix rows, then its own rows up to the query)."""
    keys = list(range(pf, pf + pl)) + list(range(first, first + n))
    mask = np.arange(len(keys))[None, :] <= pl + np.arange(n)[:, None]
    out = np.zeros((n, heads * d), F64)
    for h in range(heads):
        g = h // (heads // kvh)
        qh = q[first:first + n, h * d:(h + 1) * d].astype(F64)
        kh, vh = k[keys, g * d:(g + 1) * d].astype(F64), v[keys, g * d:(g + 1) * d].astype(F64)
        s = np.where(mask, qh @ kh.T / np.sqrt(d), -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[:, h * d:(h + 1) * d] = (p / p.sum(-1, keepdims=True)) @ vh
    return out


@pytest.mark.parametrize("d,group,ps", ATT_CASES, ids=lambda x: f"{x[0]}+{'-'.join(map(str, x[1]))}" if isinstance(x, tuple) else str(x))
def test_prefix_attention_against_float64(d, group, ps):
    from kjarni_amd import ops
    prefix, rems = ps
    heads, kvh, T, q, k, v, ctx, table = _att_inputs(d, group, prefix, rems, d * 100 + group * 10 + prefix)
    got = ops.packed_prefix_attention(q, k, v, table, heads, kvh, d, ctx=ctx)
    for first, n, pf, pl in table:
        _within(got[first:first + n, :heads * d], _att_ref(q, k, v, first, n, pf, pl, heads, kvh, d), f"d {d} group {group} prefix {pl} rows {n}")
    # the other group's rows, the prefix's own rows, the rows at or past the end and the padding columns: bit for bit what they were
    own = 2 + prefix
    assert np.array_equal(_bits(got[:own]), _bits(ctx[:own])) and np.array_equal(_bits(got[T:]), _bits(ctx[T:]))
    assert np.array_equal(_bits(got[:, heads * d:]), _bits(ctx[:, heads * d:]))


@pytest.mark.parametrize("d", [16, 32, 64, 128])
def test_prefix_attention_equals_the_packed_kernel_on_the_concatenation(d):
    """packed_attention_kernel (the 32-query route of ops.packed_causal_attention) run on [prefix; remainder] as one sequence:
    rows prefix_len .. are the remainder's rows, bit for bit; and with no prefix the two kernels agree on whole sequences."""
    from kjarni_amd import ops
    for prefix, rems in PREFIX_SETS:
        heads, kvh, T, q, k, v, ctx, table = _att_inputs(d, 2, prefix, rems, 31 + d + prefix)
        got = ops.packed_prefix_attention(q, k, v, table, heads, kvh, d, ctx=ctx)
        for first, n, pf, pl in table:
            assert pl + n < 256                                                     # (the concatenation stays on the 32-query route)
            cat = [np.concatenate([x[pf:pf + pl], x[first:first + n]]) for x in (q, k, v)]
            want = ops.packed_causal_attention(*cat, [pl + n], heads, kvh, d)
            assert np.array_equal(_bits(got[first:first + n, :heads * d]), _bits(want[pl:, :heads * d])), f"d {d} prefix {pl} rows {n}"
    lengths = [1, 31, 32, 33, 70]
    rng = np.random.default_rng(d)
    rows = sum(lengths) + 2
    q, k, v = (rng.standard_normal((rows, w)).astype(np.float32) for w in (4 * d + 4, 2 * d + 8, 2 * d))
    starts = np.concatenate([[0], np.cumsum(lengths)])
    got = ops.packed_prefix_attention(q, k, v, [(int(starts[i]), n, 0, 0) for i, n in enumerate(lengths)], 4, 2, d)
    assert np.array_equal(_bits(got), _bits(ops.packed_causal_attention(q, k, v, lengths, 4, 2, d)))


@pytest.mark.parametrize("d,ps", [(32, (31, [1, 32, 33])), (64, (65, [70, 3])), (128, (200, [7, 40]))], ids=str)
def test_prefix_attention_reads_its_prefix_and_its_own_rows_only(d, ps):
    """Every Q, K and V row outside (prefix, this remainder) set to NaN -- the siblings, the other group's rows, the rows past the
    end: the remainder's rows come out finite and bit for bit as in the clean run."""
    from kjarni_amd import ops
    prefix, rems = ps
    heads, kvh, T, q, k, v, ctx, table = _att_inputs(d, 2, prefix, rems, 7 + d)
    clean = ops.packed_prefix_attention(q, k, v, table, heads, kvh, d, ctx=ctx)
    for first, n, pf, pl in table:
        qn, kn, vn = (np.full_like(x, np.nan) for x in (q, k, v))
        for dst, src in ((qn, q), (kn, k), (vn, v)):
            dst[pf:pf + pl] = src[pf:pf + pl]
            dst[first:first + n] = src[first:first + n]
        got = ops.packed_prefix_attention(qn, kn, vn, table, heads, kvh, d, ctx=ctx)
        assert np.isfinite(got[first:first + n]).all(), f"remainder at row {first}: NaN leaked in"
        assert np.array_equal(_bits(got[first:first + n]), _bits(clean[first:first + n])), f"remainder at row {first} changed with its neighbours"


def test_hooks_validate():
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    q, kv = np.zeros((12, 64), np.float32), np.zeros((12, 32), np.float32)
    ok = dict(remainders=[(4, 3, 0, 4), (7, 5, 0, 4)], heads=2, kv_heads=1, head_dim=32)
    ops.packed_prefix_attention(q, kv, kv, **ok)
    for kw, words in ((dict(remainders=[(4, 9, 0, 4)]), "remainders[0]"), (dict(remainders=[(4, 3, 0, 4), (-1, 2, 0, 4)]), "remainders[1]"),
                      (dict(remainders=[(4, 3, 10, 4)]), "prefix rows"), (dict(remainders=[(4, 3, 2, 4)]), "overlaps"),
                      (dict(remainders=[(4, 3, 5, 1)]), "overlaps"), (dict(remainders=[(4, 0, 0, 4)]), "remainders[0]"),
                      (dict(head_dim=24), "head_dim"), (dict(heads=3, kv_heads=2), "heads")):
        with pytest.raises(KjarniException) as e:
            ops.packed_prefix_attention(q, kv, kv, **(ok | kw))
        assert e.value.code == E.INVALID_CONFIG and words in str(e.value), str(e.value)
    with pytest.raises(KjarniException) as e:      # a leading dimension that is no multiple of 4
        ops.packed_prefix_attention(np.zeros((12, 66), np.float32), kv, kv, **ok)
    assert e.value.code == E.INVALID_CONFIG and "multiples of 4" in str(e.value)
    x, g = np.ones((5, 32), np.float32), np.ones(32, np.float32)
    ops.score_gather_norm(x, [0, 4, 4], g)
    for src in ([5], [-1], [0, 1, 7]):
        with pytest.raises(KjarniException) as e:
            ops.score_gather_norm(x, src, g)
        assert e.value.code == E.INVALID_CONFIG and "src[" in str(e.value)
    with pytest.raises(KjarniException) as e:      # an odd leading dimension of the output
        ops.score_gather_norm(x, [0], g, out=np.zeros((1, 33), np.float32))
    assert e.value.code == E.INVALID_CONFIG and "ldo" in str(e.value)


# ---- 2. gather + norm alone ------------------------------------------------------------------------------------------------------

def _gather_case(hidden):
    rng = np.random.default_rng(hidden)
    lengths = [3, 4, 1, 5]                                 # last rows 2, 6, 7, 12
    x = (rng.standard_normal((sum(lengths) + 2, hidden + 4)) * 3.0).astype(np.float32)
    x[7, :] = 0.0                                          # an all-zero row
    gamma = (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(hidden)).astype(np.float32)
    src = [12, 2, 2, 7, 6, 0, 12, 13]                      # repeats, the zero row, rows no sequence ends at
    return lengths, x, gamma, beta, src


@pytest.mark.parametrize("hidden", [100, 384, 1024])
@pytest.mark.parametrize("form", ["rms", "layernorm"])
def test_gather_norm_against_float64(hidden, form):
    from kjarni_amd import ops
    lengths, x, gamma, beta, src = _gather_case(hidden)
    eps = 1e-6 if form == "rms" else 1e-5
    out = np.full((len(src), hidden + 8), CANARY, np.float32)
    got = ops.score_gather_norm(x, src, gamma, beta if form == "layernorm" else None, eps, out=out)
    rows = x[src, :hidden].astype(F64)
    if form == "rms":
        ref = rows / np.sqrt((rows * rows).mean(-1, keepdims=True) + eps) * gamma.astype(F64)
    else:
        mu = rows.mean(-1, keepdims=True)
        ref = (rows - mu) / np.sqrt(((rows - mu) ** 2).mean(-1, keepdims=True) + eps) * gamma.astype(F64) + beta.astype(F64)
    _within(got[:, :hidden], ref, f"gather {form} hidden {hidden}")
    assert np.array_equal(_bits(got[:, hidden:]), _bits(out[:, hidden:]))                        # the padding columns
    assert np.array_equal(got[3, :hidden], np.zeros(hidden, np.float32) if form == "rms" else beta)
    assert np.array_equal(_bits(got[1]), _bits(got[2])) and np.array_equal(_bits(got[0]), _bits(got[6]))


@pytest.mark.parametrize("hidden", [100, 384, 1024, 1280])
def test_gather_norm_follows_the_existing_kernels_bit_for_bit(hidden):
    """RMS form: last_token_pool_kernel without its L2 step (ops.last_token_pool, normalize=False) on the rows sequences end at.
    LayerNorm form: launch_layernorm (ops.layer_norm) on the gathered rows -- the float4 kernel up to 1 024 columns, the generic one
    beyond."""
    from kjarni_amd import ops
    lengths, x, gamma, beta, src = _gather_case(hidden)
    ends = (np.cumsum(lengths) - 1).tolist()
    pooled = ops.last_token_pool(x, lengths, gamma, 1e-6, normalize=False)
    picks = [12, 2, 2, 7, 6, 12]
    got = ops.score_gather_norm(x, picks, gamma, None, 1e-6)
    assert np.array_equal(_bits(got), _bits(pooled[[ends.index(r) for r in picks]]))
    got = ops.score_gather_norm(x, src, gamma, beta, 1e-5)
    want = ops.layer_norm(np.ascontiguousarray(x[src, :hidden]), gamma, beta, 1e-5)[0]
    assert np.array_equal(_bits(got), _bits(want))


# ---- 3. whole models -----------------------------------------------------------------------------------------------------------------

MODELS = [("llama", False), ("llama", True), ("qwen2", False), ("qwen2", True), ("gpt2", False), ("gpt2", True), ("Q3_SMALL", False),
          ("Q3_D128", True)]
MODEL_IDS = [f"{k}{'-bf16' if b else ''}" for k, b in MODELS]
INDEPENDENT = ([5, 2, 30, 9, 64, 24, 100], [1, 1, 15, 8, 1, 23, 60])
CONTEXTS, CONTINUATIONS = (40, 33, 64), (1, 3, 8, 17)


class _Case:
    """A decoder, its float64 logits per sequence (computed once per sequence), the id range."""

    def __init__(self, tmp_path, kind, bf16, **over):
        if kind.startswith("Q3"):
            import kjarni_amd
            from tests.qwen3_ref64 import Qwen3Ref64
            d = str(tmp_path / f"{kind}-{int(bf16)}")
            cfg, t = F.qwen3_model(d, getattr(F, kind), seed=F.MODEL_SEED, store_bf16=bf16, **over)
            self.dec, ref = kjarni_amd.HipDecoder(d), Qwen3Ref64(t, cfg)
            self.first_id, self.vocab = 4, cfg["vocab_size"]
            self._logits = lambda ids: ref.logits(ref.forward(list(ids), ref.new_cache()))
        else:
            self.dec, ref = _model(tmp_path, kind, bf16, **over)
            self.first_id, self.vocab = ref.first_id, ref.vocab
            self._logits = lambda ids: ref.logits(list(ids), ref.new())
        assert self.dec.bf16 == bf16
        self._cache = {}

    def logits(self, ids):
        key = tuple(ids)
        if key not in self._cache:
            self._cache[key] = np.asarray(self._logits(ids), F64)
        return self._cache[key]

    def independent(self):
        rng = np.random.default_rng(21)
        return [rng.integers(self.first_id, self.vocab, n).tolist() for n in INDEPENDENT[0]], list(INDEPENDENT[1])

    def shared(self):
        rng = np.random.default_rng(22)
        seqs, firsts = [], []
        for c in CONTEXTS:
            ctx = rng.integers(self.first_id, self.vocab, c).tolist()
            for n in CONTINUATIONS:
                seqs.append(ctx + rng.integers(self.first_id, self.vocab, n).tolist())
                firsts.append(c)
        return seqs, firsts


def _split(flat, seqs, firsts):
    return np.split(flat, np.cumsum([len(s) - f for s, f in zip(seqs, firsts)])[:-1])


def _check_sequence(got, logits64, targets, what, bar_factor=2.0, every_row=True):
    """got = (logprob, top, top_logprob) of rows whose float64 logits are logits64: 2B on the values, the arg-max on every row
    (every_row False: on the rows whose two best float64 logits are lanes_cases.GAP apart; returns how many were left out)."""
    lp, top, tlp = got
    rows = logits64.shape[0]
    assert lp.shape == top.shape == tlp.shape == (rows,), what
    lsm, _ = _log_softmax64(logits64)
    bar = bar_factor * _bar(logits64)
    want_top = _last_max_rows(logits64)
    for name, g, w in (("logprob", lp, lsm[np.arange(rows), np.asarray(targets, np.int64)]), ("top_logprob", tlp, lsm[np.arange(rows), want_top])):
        err = float(np.abs(np.asarray(g, F64) - w).max())
        print(f"{what}: {name} err {err:.3e} bar {bar:.3e}")
        assert np.isfinite(g).all() and err <= bar, f"{what}: {name}: {err:.3e} > {bar:.3e}"
    clear = _gaps(logits64) >= LC.GAP
    if every_row:
        assert clear.all(), f"{what}: precondition: a row's two best float64 logits lie within {LC.GAP}"
    assert (top.astype(np.int64)[clear] == want_top[clear]).all(), f"{what}: arg-max"
    return int(rows - clear.sum())


def _check_batch(case, seqs, firsts, what, got=None, every_row=True):
    """score_batch(seqs, firsts) against float64, sequence by sequence; returns the per-sequence (logprob, top, top_logprob).
    every_row False (batches whose rows nobody counted on the CPU): tests/test_gpu_score.py's rule, at most 2 % of the rows may
    be left out of the arg-max comparison for a near tie, none below 50 rows."""
    lp, tid, tlp = case.dec.score_batch(seqs, firsts) if got is None else got
    assert tid.shape == tlp.shape == (lp.size, 1)
    per = list(zip(_split(lp, seqs, firsts), _split(tid[:, 0], seqs, firsts), _split(tlp[:, 0], seqs, firsts)))
    left_out = 0
    for i, (s, f) in enumerate(zip(seqs, firsts)):
        left_out += _check_sequence(per[i], case.logits(s)[f - 1:len(s) - 1], s[f:], f"{what} sequence {i} ({len(s)} tokens, first {f})",
                                    every_row=every_row)
    assert left_out <= (0 if lp.size < 50 else int(0.02 * lp.size)), f"{what}: {left_out} of {lp.size} rows have their two best logits within {LC.GAP}"
    return per


def _close(a, b, logits64, what, factor=4.0):
    """Two device results of the same rows: within 4B."""
    bar = factor * _bar(logits64)
    for name, x, y in (("logprob", a[0], b[0]), ("top_logprob", a[2], b[2])):
        err = float(np.abs(np.asarray(x, F64) - np.asarray(y, F64)).max())
        assert err <= bar, f"{what}: {name}: {err:.3e} > {bar:.3e}"
    assert np.array_equal(a[1], b[1]), f"{what}: arg-max"


@pytest.mark.parametrize("kind,bf16", MODELS, ids=MODEL_IDS)
def test_models_against_float64(tmp_path, kind, bf16):
    import kjarni_amd
    case = _Case(tmp_path, kind, bf16)
    dec = case.dec
    # independent sequences: nothing shared, nothing saved
    seqs, firsts = case.independent()
    plan = kjarni_amd.score_plan(seqs, firsts, dec.head_dim)
    assert len(plan["groups"]) == 0
    r0, f0 = dec.score_batch_rows(), dec.score_calls()
    per = _check_batch(case, seqs, firsts, f"{kind} independent")
    r1, f1 = dec.score_batch_rows(), dec.score_calls()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (sum(INDEPENDENT[0]), 0)
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (1, 0)                                   # one fused head launch for the whole chunk
    for i, (s, f) in enumerate(zip(seqs, firsts)):
        _close(per[i], dec.score(s, f), case.logits(s)[f - 1:len(s) - 1], f"{kind} independent sequence {i} against score() alone")
    # shared contexts: every context computed once
    seqs, firsts = case.shared()
    plan = kjarni_amd.score_plan(seqs, firsts, dec.head_dim)
    assert [tuple(g) for g in plan["groups"].tolist()] == [(0, 4 * i, 4, c) for i, c in enumerate(CONTEXTS)]
    r0 = dec.score_batch_rows()
    per = _check_batch(case, seqs, firsts, f"{kind} shared")
    r1 = dec.score_batch_rows()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (sum(CONTEXTS) + 3 * sum(CONTINUATIONS), 3 * sum(CONTEXTS))
    for i, (s, f) in enumerate(zip(seqs, firsts)):
        _close(per[i], dec.score(s, f), case.logits(s)[f - 1:len(s) - 1], f"{kind} shared sequence {i} against score() alone")
    # the same sequences interleaved by context: neighbours share nothing, the results are the same inside the bars
    order = [4 * c + k for k in range(4) for c in range(3)]
    mixed, mixed_firsts = [seqs[i] for i in order], [firsts[i] for i in order]
    r0 = dec.score_batch_rows()
    per_mixed = _check_batch(case, mixed, mixed_firsts, f"{kind} interleaved")
    r1 = dec.score_batch_rows()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (sum(len(s) for s in seqs), 0)
    for slot, i in enumerate(order):
        _close(per_mixed[slot], per[i], case.logits(seqs[i])[firsts[i] - 1:len(seqs[i]) - 1], f"{kind} sequence {i}: shared against not shared")


# ---- 4. chunks, the matrix-core prefix, the tile route ---------------------------------------------------------------------------------

def test_more_rows_than_a_chunk(tmp_path):
    """30 sequences of 60 .. 120 tokens and a 4-way group (context 100; continuations 30, 40, 50, 60: 280 rows) put where the first
    chunk has fewer rows left than that: the chunk closes before the group."""
    import kjarni_amd
    case = _Case(tmp_path, "llama", False)
    rng = np.random.default_rng(17)
    lengths = rng.integers(60, 121, 30).tolist()
    assert sum(lengths) > 2048
    seqs = [rng.integers(case.first_id, case.vocab, n).tolist() for n in lengths]
    firsts = [int(rng.integers(1, n)) for n in lengths]
    at = int(np.searchsorted(np.cumsum(lengths), 2048, side="right"))       # the first sequence the first chunk does not hold
    ctx = rng.integers(case.first_id, case.vocab, 100).tolist()
    group = [ctx + rng.integers(case.first_id, case.vocab, n).tolist() for n in (30, 40, 50, 60)]
    seqs[at:at] = group
    firsts[at:at] = [100] * 4
    plan = kjarni_amd.score_plan(seqs, firsts, case.dec.head_dim)
    assert len(plan["chunk_rows"]) >= 2 and plan["chunk_first_seq"][1] == at and 2048 - plan["chunk_rows"][0] < 280
    assert (1, at, 4, 100) in [tuple(g) for g in plan["groups"].tolist()]
    r0 = case.dec.score_batch_rows()
    _check_batch(case, seqs, firsts, "chunks", every_row=False)
    r1 = case.dec.score_batch_rows()
    assert r1[0] - r0[0] == int(plan["chunk_rows"].sum()) and r1[1] - r0[1] >= 300


def test_prefix_on_the_matrix_core_route(tmp_path):
    import kjarni_amd
    case = _Case(tmp_path, "Q3_D128", False, max_position_embeddings=320)
    rng = np.random.default_rng(23)
    ctx = rng.integers(case.first_id, case.vocab, 260).tolist()
    seqs = [ctx + rng.integers(case.first_id, case.vocab, n).tolist() for n in (5, 12, 20)]
    firsts = [260] * 3
    plan = kjarni_amd.score_plan(seqs, firsts, case.dec.head_dim)
    assert [tuple(g) for g in plan["groups"].tolist()] == [(0, 0, 3, 260)]
    assert [tuple(b) for b in plan["mfma"].tolist()] == [(0, 0, q0, 260) for q0 in (0, 128, 256)] and len(plan["vec"]) == 0
    assert len(plan["prefix"]) == 3
    r0 = case.dec.score_batch_rows()
    _check_batch(case, seqs, firsts, "matrix-core prefix", every_row=False)
    r1 = case.dec.score_batch_rows()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (260 + 37, 520)


def test_reaches_the_tile_route(tmp_path):
    """The 1 600-row case of test_gpu_decoder_embed.test_embed_reaches_the_tile_route, scored from position 1 590."""
    case = _Case(tmp_path, "Q3_06B_WIDTHS", False, max_position_embeddings=2048)
    rng = np.random.default_rng(4)
    seqs = [rng.integers(4, case.vocab, 1600).tolist(), rng.integers(4, case.vocab, 40).tolist()]
    firsts = [1590, 1]
    before = case.dec.tile_gemm_calls()
    got = case.dec.score_batch(seqs, firsts)
    assert case.dec.tile_gemm_calls() - before == 3 * case.dec.layers
    _check_batch(case, seqs, firsts, "tile route", got=got, every_row=False)


# ---- 5. top-k ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", [True, False], ids=["fused", "rows"])
def test_top_k(tmp_path, fused):
    case = _Case(tmp_path, "llama", False)
    dec = case.dec
    dec.set_score_fused(fused)
    seqs, firsts = case.shared()
    f0 = dec.score_calls()
    lp1, tid1, tlp1 = dec.score_batch(seqs, firsts, 1)
    f1 = dec.score_calls()
    lp8, tid8, tlp8 = dec.score_batch(seqs, firsts, 8)
    rows = lp1.size
    assert (f1[0] - f0[0], f1[1] - f0[1]) == ((1, 0) if fused else (0, -(-rows // 8)))
    assert tid8.shape == tlp8.shape == (rows, 8)
    assert _same_bits(lp1, lp8), "logprob differs between top_k 1 and 8"
    assert np.array_equal(tid1[:, 0], tid8[:, 0]) and _same_bits(np.ascontiguousarray(tlp1[:, 0]), np.ascontiguousarray(tlp8[:, 0])), "slot 0"
    logits = np.concatenate([case.logits(s)[f - 1:len(s) - 1] for s, f in zip(seqs, firsts)])
    targets = np.concatenate([s[f:] for s, f in zip(seqs, firsts)])
    _check_topk((lp8, tid8, tlp8, None), logits, targets, 8, f"top_k 8 fused {fused}")
    _check_batch(case, seqs, firsts, f"top_k 1 fused {fused}", got=(lp1, tid1, tlp1))


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------

def test_leaves_generation_state_untouched(tmp_path):
    case = _Case(tmp_path, "llama", False)
    dec = case.dec
    rng = np.random.default_rng(9)
    prompt = rng.integers(4, case.vocab, 30).tolist()
    seqs, firsts = case.shared()
    first = dec.generate(prompt, 8)
    scored = dec.score(prompt, 5)
    state = (dec.cache_len(), dec.resident(), _bits(dec.last_logits()).copy(), dec.prefix_stats())
    kv = [tuple(a.copy() for a in dec.kv_rows(i)) for i in range(dec.layers)]
    dec.score_batch(seqs, firsts, 8)
    assert (dec.cache_len(), dec.resident()) == state[:2] and np.array_equal(_bits(dec.last_logits()), state[2])
    assert dec.prefix_stats() == state[3]
    for i in range(dec.layers):
        k, v = dec.kv_rows(i)
        assert np.array_equal(_bits(k), _bits(kv[i][0])) and np.array_equal(_bits(v), _bits(kv[i][1]))
    assert dec.generate(prompt, 8) == first
    again = dec.score(prompt, 5)
    assert all(np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b) for a, b in zip(scored, again))
    # prefix reuse: the kept-row counters advance by what they advance without a score_batch call in between
    dec.set_prefix_reuse(True)
    dec.generate(prompt, 8)
    s0 = dec.prefix_stats()
    second = dec.generate(prompt, 8)
    s1 = dec.prefix_stats()
    dec.score_batch(seqs, firsts)
    assert dec.prefix_stats() == s1
    assert dec.generate(prompt, 8) == second
    s2 = dec.prefix_stats()
    assert (s2[0] - s1[0], s2[1] - s1[1]) == (s1[0] - s0[0], s1[1] - s0[1]) and s1[0] - s0[0] == len(prompt) - 1


# ---- 7. validation and refusals ------------------------------------------------------------------------------------------------------

def test_validates_before_any_gpu_work(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    dec, ref = _model(tmp_path, "qwen2", False)               # max_position_embeddings 128: the length limit
    V = ref.vocab
    ids = np.arange(4, 4 + 200, dtype=np.uint32) % (V - 4) + 4
    dec.forward([5, 6, 7], fetch=False)
    cases = [
        (ids, [0, 5, 3, 9], [1, 1, 1], 1, ("offsets[2]", "sequence 1")),            # offsets that decrease
        (ids, [0, 5, 6, 9], [1, 1, 1], 1, ("fewer than 2", "sequence 1")),          # a sequence of one token
        (ids, [0, 5, 5, 9], [1, 1, 1], 1, ("fewer than 2", "sequence 1")),          # an empty one
        (ids, [0, 5, 134], [1, 1], 1, ("offsets", "129", "128", "sequence 1")),     # longer than min(context, 2048)
        (ids, [-1, 3], [1], 1, ("offsets[0]",)),
        (ids, [0, 5, 9], [1, 0], 1, ("firsts[1]", "sequence 1")),
        (ids, [0, 5, 9], [1, 4], 1, ("firsts[1]", "sequence 1")),
        (ids, [0, 5, 9], [-2, 1], 1, ("firsts[0]", "sequence 0")),
        (ids, [0, 5, 9], [1, 1], 0, ("top_k",)),
        (ids, [0, 5, 9], [1, 1], 9, ("top_k",)),
    ]
    bad = ids.copy()
    bad[7] = V
    cases.append((bad, [0, 5, 9], [1, 1], 1, ("ids[7]", str(V), "sequence 1")))
    before = (dec.score_batch_rows(), dec.score_calls(), dec.tile_gemm_calls())
    for a, off, firsts, top_k, words in cases:
        with pytest.raises(KjarniException) as e:
            dec.score_batch_flat(a, off, firsts, top_k)
        assert e.value.code == E.INVALID_CONFIG and all(w in str(e.value) for w in words), str(e.value)
    assert dec.cache_len() == 3 and (dec.score_batch_rows(), dec.score_calls(), dec.tile_gemm_calls()) == before
    lp, tid, tlp = dec.score_batch([], [])
    assert lp.shape == (0,) and tid.shape == (0, 1) and dec.score_batch_rows() == before[0]
    assert dec.score_batch_flat(ids, [0, 128], [1])[0].shape == (127,)                # exactly the limit is fine
    lp, tid, tlp = dec.score_batch_flat(ids, [0, 5, 9], [1, 3])
    check = (C.c_float * 5)()                                                           # null outputs: the others still arrive
    i32 = lambda x: np.ascontiguousarray(x, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    from kjarni_amd import _ffi
    _ffi.check_error(_ffi.lib().kjarni_hip_decoder_score_batch(dec._h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), i32([0, 5, 9]), 2, i32([1, 3]), 1,
                                                               check, None, None))
    assert np.array_equal(_bits(np.array(check[:], np.float32)), _bits(lp))


def test_refuses_quantized_and_odd_geometries_and_runs_gpt2(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    path = str(tmp_path / "q8.gguf")
    GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    dec = kjarni_amd.HipDecoder(path)
    with pytest.raises(KjarniException) as e:
        dec.score_batch([[5, 6, 7]], [1])
    assert e.value.code == E.INVALID_CONFIG and "quantized" in str(e.value) and dec.score_batch_rows() == (0, 0)
    d = str(tmp_path / "odd")      # hidden 48: not a multiple of 32, a geometry forward() keeps off the matrix-core route
    synth.llm_model(d, dict(synth.LLAMA_TEST, hidden_size=48, num_attention_heads=3, num_key_value_heads=1, head_dim=16, intermediate_size=96), seed=3)
    dec = kjarni_amd.HipDecoder(d)
    with pytest.raises(KjarniException) as e:
        dec.score_batch([[5, 6, 7]], [1])
    assert e.value.code == E.INVALID_CONFIG and "multiples of 32" in str(e.value) and dec.score_batch_rows() == (0, 0)
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**G.SMALL), seed=1)
    lp, tid, tlp = kjarni_amd.HipDecoder(d).score_batch([[5, 6, 7], [5, 6, 9, 11]], [1, 2])
    assert lp.shape == (4,) and np.isfinite(lp).all() and (lp < 0).all()


# ---- 8. the Generator ------------------------------------------------------------------------------------------------------------------

PAIRS = [("The quick brown fox", " jumps over the lazy dog"), ("The quick brown fox", " sleeps"), ("The quick brown fox", " runs away from the dog"),
         ("Hello", " world"), ("", "In a hole in the ground there lived"), ("Once upon a time there was a small", " house"),
         ("Once upon a time there was a small", " dog in the house")]


def test_generator_score_batch(tmp_path):
    from kjarni_amd import Generator, HipDecoder, _ffi
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "gpt2")
    cfg = G.gpt2_config(**dict(G.SMALL, n_ctx=128))
    _, t = G.gpt2_model(d, cfg, seed=4, tokenizer=True)
    gen, dec = Generator("gpt2", model_path=d), HipDecoder(d, 0)
    from tests.test_gpu_lookup import _Gpt264
    ref = _Gpt264(t, cfg)
    got = gen.score_batch(PAIRS)
    assert len(got) == len(PAIRS)
    for (context, continuation), (s, cnt, greedy) in zip(PAIRS, got):
        whole, first = gen.encode(context + continuation), len(gen.encode(context))
        alone = gen.score(context, continuation)
        assert cnt == len(whole) - first == alone[1] and greedy == alone[2]
        logits = np.asarray(ref.logits(whole, ref.new()), F64)[first - 1:len(whole) - 1]
        assert abs(s - alone[0]) <= 4 * _bar(logits) * cnt, (context, continuation)
    whole = [gen.encode(c + k) for c, k in PAIRS]
    firsts = [len(gen.encode(c)) for c, _ in PAIRS]
    lp = dec.score_batch(whole, firsts)[0]                                               # the same packed call, token by token
    for (s, _, _), part in zip(got, _split(lp, whole, firsts)):
        total = 0.0
        for v in part:
            total += float(v)
        assert s == total
    assert gen.score_batch([]) == []
    # an invalid pair in the middle: the whole call fails with its index, and nothing is written
    L = _ffi.lib()
    out = (_ffi.KjarniScoreResult * 3)()
    for r in out:
        r.sum_logprob, r.n_tokens, r.is_greedy = 7.0, 7, 7
    ctx = (C.c_char_p * 3)(b"Hello", b"Hello", b"Hello")
    cont = (C.c_char_p * 3)(b" world", b"", b" there")
    with pytest.raises(KjarniException, match="adds no tokens") as e:
        _ffi.check_error(L.kjarni_generator_score_batch(gen._handle, ctx, cont, 3, out))
    assert e.value.code == E.INVALID_CONFIG and "pair 1" in str(e.value)
    assert all((r.sum_logprob, r.n_tokens, r.is_greedy) == (7.0, 7, 7) for r in out)
    long = " the" * 200
    with pytest.raises(KjarniException, match="context of") as e:
        gen.score_batch([("Hello", " world"), ("Hi", " there"), ("Hello", long)])
    assert e.value.code == E.INVALID_CONFIG and "pair 2" in str(e.value)


def test_generator_score_batch_on_a_checkpoint_the_packed_path_refuses(tmp_path):
    """n_embd 48: score_batch refuses the geometry, so every pair takes score()'s own route and the results are score()'s exactly."""
    from kjarni_amd import Generator, HipDecoder
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "gpt2-48")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_embd=48, n_head=3, n_ctx=128)), seed=4, tokenizer=True)
    with pytest.raises(KjarniException, match="multiples of 32"):
        HipDecoder(d, 0).score_batch([[5, 6, 7]], [1])
    gen = Generator("gpt2", model_path=d)
    assert gen.score_batch(PAIRS) == [gen.score(c, k) for c, k in PAIRS]
