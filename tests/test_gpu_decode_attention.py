"""The decode attention (decode_attention_partial_kernel) and its three merges -- decode_attention_combine_kernel,
gemv_row_att_kernel and the slab branch of the LLM streaming GEMV -- alone, through kjarni_hip_op_decode_attention /
_gemv_row_att / _llm_gemv_att, against the float64 reference of tests/decode_attention_ref64.py.

Inputs are standard normal (bar 1e-5 absolute: the context is a convex combination of O(1) values, the bar of the encoder
attention in test_gpu_ops.py) or, for the stress cases, built so that every score is exact in float32 (asserted on the CPU),
which lets scores sit at +-60 under the same bar.  In every case the K / V rows behind the last key, the padding columns, the
scratch and the output are NaN beforehand and the result must be finite: the kernel clamps its over-reads to the last key and
must never use them.  The projections' bar is 1e-5 * max(1, max |ref|), the bar of the linear tests."""
import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import ops
from tests import decode_attention_ref64 as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
NEG_INF = np.float32(-np.inf)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def _kv(rng, counts, alloc, kvd, ld=None, interleaved=False):
    """A K or V buffer for len(counts) sequences of `alloc` rows each, row stride `ld` (default kvd); sequence s holds counts[s]
    standard-normal rows, everything else -- later rows, padding columns -- is NaN.  Blocked: sequence s starts at s * alloc * ld,
    rows ld apart.  Interleaved (Whisper's lanes): row t of sequence s is buffer row t * lanes + s, rows lanes * ld apart.
    Returns (flat buffer, row stride, lane stride)."""
    lanes = len(counts)
    ld = kvd if ld is None else ld
    buf = np.full((lanes, alloc, ld), np.nan, np.float32)
    for s, n in enumerate(counts):
        buf[s, :n, :kvd] = rng.standard_normal((n, kvd)).astype(np.float32)
    if interleaved:
        return np.ascontiguousarray(buf.transpose(1, 0, 2)).reshape(-1), lanes * ld, ld
    return buf.reshape(-1), ld, alloc * ld


def _q(rng, rows, heads, d, pad=0):
    q = np.full((rows, heads * d + pad), np.nan, np.float32)
    q[:, :heads * d] = rng.standard_normal((rows, heads * d)).astype(np.float32)
    return q


def _check(got, ref, tol=TOL):
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), "the result holds NaN / inf: an over-read row, the scratch's or the output's poison was used"
    err = float(np.abs(got - ref).max())
    print(f"max |kernel - float64| = {err:.3e} (bar {tol:.1e})")
    assert err < tol, err


def _one_sequence(rng, rows, heads, d, n, splits, kv_group=1, causal_base=-1, want_slabs=False, extra_rows=3):
    kvd = ((heads - 1) // kv_group + 1) * d
    q = _q(rng, rows, heads, d)
    k, ldk, _ = _kv(rng, [n], n + extra_rows, kvd)
    v, ldv, _ = _kv(rng, [n], n + extra_rows, kvd)
    out = ops.decode_attention(q, k, v, ldk, ldv, n, heads, d, splits, causal_base=causal_base, kv_group=kv_group, want_slabs=want_slabs)
    ref = R.attention64(q, k, v, ldk, ldv, n, heads, d, causal_base=causal_base, kv_group=kv_group)
    _check(out[0] if want_slabs else out, ref)
    return out, ref, (q, k, v, ldk, ldv)


# ---- the partial kernel's paths -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [4, 8, 16, 32, 64, 128])
def test_every_head_dim(d):
    """Lanes per key 1 .. 32: the DPP row sum (d = 64) against the shuffle sums, the cross-wave sum at 32 lanes per key."""
    _one_sequence(np.random.default_rng(100 + d), 1, 3, d, 37, 2)


@pytest.mark.parametrize("d,span", [(64, 128), (64, 129), (128, 64), (128, 65), (32, 256), (32, 257), (64, 512)])
def test_both_sides_of_the_register_held_switch(d, span):
    """Two key ranges, of `span` and span - 1 keys: the range length at which the kernel leaves the register-held path for the
    looping one is 8 * 256 / (d / 4); 512 keys fill the looping path's score buffer."""
    n = 2 * span - 1
    assert (n + 1) // 2 == span
    _one_sequence(np.random.default_rng(200 + d + span), 1, 1 if span == 512 else 2, d, n, 2)


@pytest.mark.parametrize("n,splits,empty", [(1, 8, 7), (7, 8, 1), (24, 8, 0), (1025, 3, 0)],
                         ids=["one-key", "splits-minus-1", "exact-fit", "short-last-range"])
def test_empty_exact_and_short_ranges(n, splits, empty):
    assert sum(1 for sp in range(splits) if sp * ((n + splits - 1) // splits) >= n) == empty
    (got, slabs), _, _ = _one_sequence(np.random.default_rng(300 + n), 1, 2, 64, n, splits, want_slabs=True)
    chunk = (n + splits - 1) // splits
    for sp in range(splits):
        keys = max(0, min(n, (sp + 1) * chunk) - sp * chunk)
        head = slabs[0, :, sp, :4]
        if keys == 0:   # an empty range: max -inf, sum 0, a zero accumulator -- and the merge gives it no weight (checked above)
            assert (head[:, 0] == NEG_INF).all() and (head[:, 1:] == 0).all() and (slabs[0, :, sp, 4:] == 0).all()
        else:           # sum of exp(score - max) over the range: at least the maximum's own 1, at most one per key
            assert np.isfinite(slabs[0, :, sp]).all() and (head[:, 1] >= 1.0).all() and (head[:, 1] <= keys * (1 + 1e-6)).all()
            assert (head[:, 2:] == 0).all()


@pytest.mark.parametrize("splits", [1, 2, 16, 17, 64])
def test_both_forms_of_the_combine_kernel(splits):
    """Two keys per range; up to 16 ranges merge in the unrolled form, more in the loop."""
    _one_sequence(np.random.default_rng(400 + splits), 1, 2, 64, 2 * splits, splits)


@pytest.mark.parametrize("rows,n,splits,d", [(2, 7, 3, 64), (5, 12, 4, 32), (8, 21, 4, 64)])
def test_multi_row_causal(rows, n, splits, d):
    """A verify call: row s sees keys <= n - rows + s.  The last range lies wholly behind the first rows' horizon: its slab has
    max -1e9 (every score overwritten) and must weigh exactly nothing in the merge."""
    base = n - rows
    (got, slabs), ref, (q, k, v, ldk, ldv) = _one_sequence(np.random.default_rng(500 + rows), rows, 2, d, n, splits, causal_base=base,
                                                           want_slabs=True)
    _, masks = R.scores64(q, k, ldk, n, 2, d, causal_base=base)
    chunk = (n + splits - 1) // splits
    dark = [(s, sp) for s in range(rows) for sp in range(splits) if sp * chunk < n and masks[s][:, sp * chunk:min(n, (sp + 1) * chunk)].all()]
    assert dark, "no (row, range) pair has every key masked: the case does not reach the branch"
    assert masks[0].any() and not masks[rows - 1].any()                 # the last row sees every key
    for s, sp in dark:
        assert (slabs[s, :, sp, 0] == np.float32(R.MASK_VALUE)).all()
    # the mask matters: without it the reference differs
    assert np.abs(R.attention64(q, k, v, ldk, ldv, n, 2, d) - ref)[:rows - 1].max() > 1e-2


@pytest.mark.parametrize("kv_group,heads", [(1, 3), (4, 8), (7, 14)])
def test_grouped_query_heads(kv_group, heads):
    _one_sequence(np.random.default_rng(600 + kv_group), 1, heads, 32, 37, 2, kv_group=kv_group)


def test_padded_q_and_the_two_halves_of_one_buffer():
    """Whisper's cross attention: K and V are the halves of one [keys, 2H] buffer; q rows carry 8 floats of padding."""
    rng = np.random.default_rng(700)
    heads, d, n, alloc = 4, 32, 50, 53
    H = heads * d
    q = _q(rng, 1, heads, d, pad=8)
    kv = np.full((alloc, 2 * H), np.nan, np.float32)
    kv[:n] = rng.standard_normal((n, 2 * H)).astype(np.float32)
    k, v = kv.reshape(-1), kv.reshape(-1)[H:]
    got = ops.decode_attention(q, k, v, 2 * H, 2 * H, n, heads, d, 3)
    _check(got, R.attention64(q, k, v, 2 * H, 2 * H, n, heads, d))
    # the same keys in two buffers of their own: the same bits (the layout is addressing only)
    same = ops.decode_attention(q[:, :H], kv[:, :H], kv[:, H:], H, H, n, heads, d, 3)
    assert np.array_equal(got, same)


# ---- lanes and the device-held key count ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleaved", [False, True], ids=["blocked", "interleaved"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host-count", "device-count"])
def test_lock_step_lanes(interleaved, on_device):
    """lanes = rows = 3: every row attends to its own cache, no mask between the rows (a causal base is given and must be
    ignored); with the count on the device the rows see count + 1 keys."""
    rng = np.random.default_rng(800)
    lanes, heads, d, n, alloc = 3, 2, 64, 21, 24
    q = _q(rng, lanes, heads, d)
    k, ldk, ks = _kv(rng, [n] * lanes, alloc, heads * d, interleaved=interleaved)
    v, ldv, vs = _kv(rng, [n] * lanes, alloc, heads * d, interleaved=interleaved)
    got = ops.decode_attention(q, k, v, ldk, ldv, n - 1 if on_device else n, heads, d, 2, causal_base=0, keys_on_device=on_device,
                               max_keys=alloc, k_lane_stride=ks, v_lane_stride=vs, lanes=lanes)
    ref = R.attention64(q, k, v, ldk, ldv, n, heads, d, k_lane_stride=ks, v_lane_stride=vs, lanes=lanes)
    _check(got, ref)
    one_cache = R.attention64(q, k, v, ldk, ldv, n, heads, d)          # every row on lane 0's cache: not the same thing
    assert np.abs(one_cache - ref)[1:].max() > 1e-2


def test_device_count_without_lanes():
    """rows = 4 with the count on the device: keys = count + rows, causal base = count."""
    rng = np.random.default_rng(810)
    rows, heads, d, count, alloc = 4, 2, 64, 19, 26
    n = count + rows
    q = _q(rng, rows, heads, d)
    k, ldk, _ = _kv(rng, [n], alloc, heads * d)
    v, ldv, _ = _kv(rng, [n], alloc, heads * d)
    got = ops.decode_attention(q, k, v, ldk, ldv, count, heads, d, 3, causal_base=0, keys_on_device=True, max_keys=alloc)
    ref = R.attention64(q, k, v, ldk, ldv, n, heads, d, causal_base=count)
    _check(got, ref)
    assert np.abs(R.attention64(q, k, v, ldk, ldv, n, heads, d) - ref).max() > 1e-2
    # a negative causal base: no mask, whatever the count
    _check(ops.decode_attention(q, k, v, ldk, ldv, count, heads, d, 3, causal_base=-1, keys_on_device=True, max_keys=alloc),
           R.attention64(q, k, v, ldk, ldv, n, heads, d))


def test_ragged_lanes():
    """Lane s holds lane_pos[s] + 1 keys, clamped to the capacity; a dead lane writes -inf slabs and its row is exactly zero,
    without its (all-NaN) cache being read."""
    rng = np.random.default_rng(820)
    heads, kv_group, d, cap = 4, 2, 64, 16
    pos, live = [0, 5, cap - 1, cap + 3, 7], [1, 1, 1, 1, 0]
    lanes = len(pos)
    counts = [R.keys_of_row(s, cap, pos, live) for s in range(lanes)]
    assert counts == [1, 6, cap, cap, 0]
    q = _q(rng, lanes, heads, d)
    k, ldk, ks = _kv(rng, counts, cap, 2 * d)
    v, ldv, vs = _kv(rng, counts, cap, 2 * d)
    got, slabs = ops.decode_attention(q, k, v, ldk, ldv, cap, heads, d, 2, kv_group=kv_group, k_lane_stride=ks, v_lane_stride=vs, lanes=lanes,
                                      lane_pos=pos, lane_live=live, want_slabs=True)
    _check(got, R.attention64(q, k, v, ldk, ldv, cap, heads, d, kv_group=kv_group, k_lane_stride=ks, v_lane_stride=vs, lanes=lanes,
                              lane_pos=pos, lane_live=live))
    assert (got[4] == 0.0).all() and not np.signbit(got[4]).any()
    assert (slabs[4, :, :, 0] == NEG_INF).all() and (slabs[4, :, :, 1:] == 0).all()


# ---- scores far from zero --------------------------------------------------------------------------------------------------------

def _stress(d, levels, splits, causal_base, seed):
    """Run the exact-score case with and without the mask; returns the float64 scores of the unmasked run."""
    rng = np.random.default_rng(seed)
    n = len(levels)
    q, kk = R.exact_score_inputs(rng, d, levels)
    k = np.full((n + 2, 2 * d), np.nan, np.float32)
    k[:n] = kk
    v, ldv, _ = _kv(rng, [n], n + 2, 2 * d)
    k = k.reshape(-1)
    sc64, _ = R.scores64(q, k, 2 * d, n, 2, d)
    sc32, _ = R.scores64(q, k, 2 * d, n, 2, d, dtype=np.float32)
    assert sc32[0].dtype == np.float32 and np.array_equal(sc32[0].astype(np.float64), sc64[0]), "the scores are not exact in float32"
    assert np.abs(sc64[0]).max() <= 72.0
    ref = R.attention64(q, k, v, 2 * d, ldv, n, 2, d)
    _check(ops.decode_attention(q, k, v, 2 * d, ldv, n, 2, d, splits), ref)
    masked = R.attention64(q, k, v, 2 * d, ldv, n, 2, d, causal_base=causal_base)
    assert np.abs(masked - ref).max() > 1e-2, "masking the dominant keys does not change the reference: the branch would not matter"
    _check(ops.decode_attention(q, k, v, 2 * d, ldv, n, 2, d, splits, causal_base=causal_base), masked)
    return sc64[0]


@pytest.mark.parametrize("d", [4, 16, 64])
@pytest.mark.parametrize("at", [2, 13, 23], ids=["first-range", "middle-range", "last-range"])
def test_one_key_far_above_the_rest(d, at):
    """24 keys in 4 ranges, one of them 40 above the rest: the other ranges' weights are exp(-40); then that key (and the ones
    behind it) masked."""
    levels = np.zeros(24)
    levels[at] = 40.0
    sc = _stress(d, levels, 4, at - 1, 900 + d + at)
    assert (sc[:, at] - np.delete(sc, at, axis=1).max(axis=1) > 30).all()


@pytest.mark.parametrize("d", [4, 16, 64])
@pytest.mark.parametrize("low", [0, 2])
def test_a_range_whose_weight_underflows(d, low):
    """One range's maximum lies more than 110 below the global one: exp(m_i - M) is 0 in float32.  Masked, the ranges behind it
    go dark and the low range carries weight."""
    levels = np.full(24, 55.0)
    levels[low * 6:(low + 1) * 6] = -60.0
    sc = _stress(d, levels, 4, (low + 1) * 6 - 1, 1000 + d + low)
    assert (sc.max(axis=1) - sc[:, low * 6:(low + 1) * 6].max(axis=1) > 110).all()


@pytest.mark.parametrize("d", [4, 16, 64])
@pytest.mark.parametrize("level", [60.0, -60.0])
def test_every_score_far_from_zero(d, level):
    """All scores near +60, or near -60: only the subtraction of the maximum keeps the exponentials in range and precise."""
    levels = np.full(24, level)
    levels[17] += 4.0                                                   # the key the masked run loses
    sc = _stress(d, levels, 4, 16, 1100 + d + int(level))
    assert (np.abs(sc - level) < 12).all()


# ---- the projections that merge the slabs --------------------------------------------------------------------------------------------

def _slabs(rng, heads, splits, d, empty=(), dead_heads=()):
    """Slabs as the attention leaves them: per (head, range) a maximum, a sum of exponentials in [1, keys] and an accumulator of
    that size; `empty` ranges are (-inf, 0, 0...), `dead_heads` have nothing but empty ranges."""
    s = np.zeros((heads, splits, d + 4), np.float32)
    s[:, :, 0] = (rng.standard_normal((heads, splits)) * 3).astype(np.float32)
    s[:, :, 1] = rng.uniform(1.0, 40.0, (heads, splits)).astype(np.float32)
    s[:, :, 4:] = s[:, :, 1:2] * (rng.standard_normal((heads, splits, d)) * 0.7).astype(np.float32)
    for sp in empty:
        s[:, sp] = 0
        s[:, sp, 0] = NEG_INF
    for h in dead_heads:
        s[h] = 0
        s[h, :, 0] = NEG_INF
    return s


def _projection_inputs(rng, k, d, splits, n_out):
    empty = () if splits == 1 else (splits // 2,)
    slabs = _slabs(rng, k // d, splits, d, empty=empty, dead_heads=(1,) if splits == 5 else ())
    w = (rng.standard_normal((n_out, k)) * 0.05).astype(np.float32)
    return slabs, w, rng.standard_normal(n_out).astype(np.float32), rng.standard_normal(n_out).astype(np.float32)


def _check_projection(got, ref):
    _check(got, ref, TOL * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("splits", [1, 5, 16])
@pytest.mark.parametrize("k,d", [(512, 64), (512, 32), (2048, 64), (2048, 128)])
def test_gemv_row_att(k, d, splits):
    """Whisper's output projection on slabs: against float64, and bit for bit against the route it replaces (the combine pass,
    then the one-row projection + bias + residual), as its source comment says."""
    for n_out in (6, 66):
        rng = np.random.default_rng(1200 + k + d + splits + n_out)
        slabs, w, bias, r = _projection_inputs(rng, k, d, splits, n_out)
        assert np.abs(R.merge64(slabs)).max() > 0.1
        for b in (bias, None):
            ref = R.merge_project64(slabs, w, b, r)
            got = ops.gemv_row_att(slabs, w, b, r, d)
            _check_projection(got, ref)
            assert np.array_equal(got, ops.gemv_row_att(slabs, w, b, r, d, two_step=True)), "differs from combine + projection"
            assert np.array_equal(got, ops.gemv_row_att(slabs, w, b, r, d, in_place=True)), "differs with the residual row as the output row"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("k,splits", [(2048, 1), (2048, 4), (2048, 8), (4096, 1), (4096, 4)])
def test_llm_gemv_att(k, splits, d, bf16):
    """The slab branch of the LLM's weight-streaming projection, f32 and bf16 weights (widened exactly in the reference)."""
    for n_out in (6, 66):
        rng = np.random.default_rng(1300 + k + d + splits + n_out)
        slabs, w, bias, r = _projection_inputs(rng, k, d, splits, n_out)
        if bf16:
            w = ops.to_bf16(w)
        for b in (bias, None):
            _check_projection(ops.llm_gemv_att(slabs, w, b, r, d, bf16=bf16), R.merge_project64(slabs, w, b, r, bf16=bf16))


def test_projections_on_the_attention_kernels_own_slabs():
    """End to end at one token: the slabs of a real attention call, merged by each projection, against float64 attention +
    projection."""
    rng = np.random.default_rng(1400)
    heads, d, n, splits, n_out = 32, 64, 41, 4, 66
    q = _q(rng, 1, heads, d)
    k, ldk, _ = _kv(rng, [n], n + 1, heads * d)
    v, ldv, _ = _kv(rng, [n], n + 1, heads * d)
    _, slabs = ops.decode_attention(q, k, v, ldk, ldv, n, heads, d, splits, want_slabs=True)
    w = (rng.standard_normal((n_out, heads * d)) * 0.05).astype(np.float32)
    r = rng.standard_normal(n_out).astype(np.float32)
    ref = w.astype(np.float64) @ R.attention64(q, k, v, ldk, ldv, n, heads, d)[0] + r
    _check_projection(ops.gemv_row_att(slabs[0], w, None, r, d), ref)
    _check_projection(ops.llm_gemv_att(slabs[0], w, None, r, d), ref)


def test_a_refusal_with_a_device_present():
    """The refusals themselves need no GPU (tests/test_decode_attention_host.py); with one present the answer is the same."""
    q = np.zeros((1, 96), np.float32)
    kv = np.zeros(96 * 4, np.float32)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        ops.decode_attention(q, kv, kv, 96, 96, 4, 1, 96, 1)
    assert e.value.code == kjarni_amd._ffi.KjarniError.INVALID_CONFIG
