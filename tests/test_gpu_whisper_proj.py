"""The Whisper decoder's row projections and the front-end kernels alone: launch_gemv_rows (gemv_row_fast_kernel and its EMBED
variant, gemv_rows_lds_fast_kernel, gemv_rows_head_kernel, gemv_rows_lds_kernel, gemv_rows_kernel, the fall-through to launch_gemm)
through kjarni_hip_op_gemv_rows, and mel_frames / mel_power / mel_log_normalize / im2col3 / add_rows / decoder_embed through their
hooks, one launch per call, against tests/whisper_proj_ref64.py at the widths, row counts and edges the whole-model tests never reach.

Every projection case
  * holds the route the launcher reports (gemv_rows_route, the function the launcher itself follows) against the Python restatement
    of the rule and against the kernel family the case is filed under, so a case that stops reaching its kernel fails;
  * pre-fills its outputs, the padding columns of x (ldx > k) and of the outputs (ldy > n_out), the rows of x past `rows` and the
    cache rows outside [row_off, row_off + rows) with one NaN bit pattern and asserts that every element the operation owns is finite
    and on the bar and that every other element still holds that pattern;
  * runs twice and asserts the same bits.
Inputs are random, scaled so that max |ref| stays O(1 - 10), or exact probes: integer weights in -7 .. 7 and an integer row whose one
large entry sits at the first or last element of a lane's chunk -- column (lane + 64 j) * 4 + c for the first and last j, lane and c --
so every sum is an integer below 2^24, any order of summation gives the same f32 and an element taken from the wrong place gives
another integer.

The bar: 1e-5 x max(1, max |ref|) against float64, the bar of test_gpu_dense_proj / test_gpu_quant_proj for wave-per-column kernels.
The front-end kernels that only move data or do one correctly rounded operation are held to the reference bit for bit.

The large-mean LayerNorm row is 1e3 + N(0, 1) with the noise rounded to sixteenths (quarters above 512 columns) and shifted to sum
to zero: f32 then holds the sum of the row and its mean, 1000, exactly, so the case tests the two-pass variance (a one-pass
E[x^2] - mean^2 loses everything at x^2 ~ 1e6) and not the f32 format.  With unrounded noise the mean is no f32: rounding the exact
mean alone shifts every normalised element by 1.4e-5 .. 2.9e-5 and the result by as much times sum(gamma * w) ~ N(0, 1), and the
f32 sum of the row (5e5, half an ulp 0.03) adds to it -- measured on the MI355X, not asserted: 1.2 .. 6.7 times this bar (errors
2.5e-5 .. 1.3e-4) on the six routes of test_layernorm_edges."""
import math

import numpy as np
import pytest

from tests import whisper_proj_ref64 as W
from tests.parity_report import report

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN_BITS = np.uint32(0x7FC01234)
BIAS, GELU, RES = W.EPI_BIAS, W.EPI_BIAS_GELU, W.EPI_BIAS_RESIDUAL
PAIRS = W.PAIRS
PNAME = {(BIAS, True): "ln+bias", (BIAS, False): "bias", (GELU, True): "ln+gelu", (RES, False): "residual"}
EPS = 1e-5


def _ops():
    from kjarni_amd import ops
    return ops


def _refused():
    from kjarni_amd._ffi import KjarniError, KjarniException
    return KjarniException, KjarniError.INVALID_CONFIG


def nans(*shape):
    return np.full(shape, NAN_BITS, np.uint32).view(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- operands, made once and never changed -----------------------------------------------------------------------------------------

_CACHE = {}


def mat(n, k, seed=0):
    """Weights [n, k] ~ N(0, 1 / k); a case that needs fewer rows slices the first ones."""
    key = ("w", n, k, seed)
    if key not in _CACHE:
        _CACHE[key] = np.random.default_rng([n, k, seed]).standard_normal((n, k), dtype=F32) * F32(1.0 / math.sqrt(k))
    return _CACHE[key]


def int_mat(n, k, salt=0):
    """Integer weights in -7 .. 7, no two neighbouring rows or columns alike."""
    key = ("i", n, k, salt)
    if key not in _CACHE:
        r, c = np.arange(n, dtype=np.int64)[:, None], np.arange(k, dtype=np.int64)[None, :]
        _CACHE[key] = (r * 31 + c * 17 + (r * c) % 7 + c // 64 + salt * 5) % 15 - 7
    return _CACHE[key]


def chunk_columns(k):
    """Column (lane + 64 j) * 4 + c for the first and last j, lane and c (k < 256: the corners of the row)."""
    k4 = k // 4
    js = sorted({0, max((k4 - 1) // 64, 0)})
    cols = []
    for j in js:
        for lane in (0, 63):
            for c in (0, 3):
                col = (lane + 64 * j) * 4 + c
                if col < k:
                    cols.append(col)
    return sorted(set(cols + [0, k - 1]))


WORST = {}


def check(group, case, got, ref, row0=0):
    """got [out_rows, ldy]: the operation owns rows row0 .. row0 + rows - 1, columns 0 .. n - 1 of it and nothing else."""
    ref = np.asarray(ref, F64)
    rows, n = ref.shape
    own = np.zeros(got.shape, bool)
    own[row0:row0 + rows, :n] = True
    assert (bits(got)[~own] == NAN_BITS).all(), f"{group} {case}: an element outside the output was written"
    val = got[row0:row0 + rows, :n]
    assert np.isfinite(val).all(), f"{group} {case}: not finite"
    err, bar = float(np.abs(val - ref).max()), W.bar(ref)
    ratio = err / bar
    if ratio >= WORST.get(group, (0.0,))[0]:
        WORST[group] = (ratio, err, bar, case)
    print(f"[whisper_proj] {group} {case}: err {err:.3e} bar {bar:.3e} ({ratio:.2f} of it)")
    report(f"whisper_proj {group}: largest err / bar", ratio, 1.0)
    assert err <= bar, f"{group} {case}: err {err:.3e} > bar {bar:.3e}"


def untouched(group, case, *arrays):
    for a in arrays:
        assert (bits(a) == NAN_BITS).all(), f"{group} {case}: an array the call does not own was written"


# ---- one launch of launch_gemv_rows ------------------------------------------------------------------------------------------------

def operands(rows, k, n_out, pair, seed=0, pads=(8, 0, 0, 0), scales=None, x_values=None, bias=True, w_rows=None):
    """(x [rows + 1, k + pad] with NaN outside the rows and columns used, w, gamma, beta, bias, r [rows, n_out + pad])."""
    epi, ln = pair
    rng = np.random.default_rng([seed, rows, k, n_out, epi, int(ln)])
    x = nans(rows + 1, k + pads[0])
    v = rng.standard_normal((rows, k)) if x_values is None else np.asarray(x_values, F64)
    if scales is not None:
        v = v * np.asarray(scales, F64)[:rows, None]
    x[:rows, :k] = v.astype(F32)
    w = mat(w_rows or max(n_out, 1), k)[:max(n_out, 1)]
    gamma = (1.0 + 0.1 * rng.standard_normal(k)).astype(F32) if ln else None
    beta = (0.1 * rng.standard_normal(k)).astype(F32) if ln else None
    b = (0.1 * rng.standard_normal(max(n_out, 1))).astype(F32) if bias else None
    r = rng.standard_normal((rows, max(n_out, 1) + pads[3])).astype(F32) if epi == RES else None
    return x, w, gamma, beta, b, r


def proj_case(group, case, want_route, *, rows, k, n_out, pair, seg=0, row_off=0, on_device=False, inplace=False, pads=(8, 0, 0, 0),
              cache_rows=6, misalign=0, raw=False, norm=False, seed=0, scales=None, x_values=None, bias=True, w_rows=None, loose_beta=False):
    """pads = (ldx - k, ldy0 - columns, ldy12 - seg, ldr - n_out).  want_route: the family the case is filed under.  loose_beta: a beta
    without gamma (no LayerNorm), which takes a 512- / 2048-float row off the fast kernels when it is misaligned.  Returns the outputs."""
    ops = _ops()
    epi, ln = pair
    x, w, gamma, beta, b, r = operands(rows, k, n_out, pair, seed, pads, scales, x_values, bias, w_rows)
    if loose_beta:
        beta = np.zeros(k, F32)
    ref = W.gemv_rows64(x[:rows, :k], w, gamma=gamma, beta=beta if ln else None, eps=EPS, bias=b, epi=epi, r=None if r is None else r[:, :n_out])
    y0 = nans(rows + 1, (seg or n_out) + pads[1])
    ys = [y0] if not seg else [y0, nans(cache_rows, seg + pads[2]), nans(cache_rows, seg + pads[2])]
    if inplace:
        y0[:rows, :n_out] = r[:, :n_out]
    kw = dict(k=k, gamma=gamma, beta=beta, eps=EPS, bias=b, r=None if inplace else r, r_is_y0=inplace, seg=seg, row_off=row_off,
              offset_on_device=on_device, epi=epi, x_raw_out=nans(k) if raw else None, x_norm_out=nans(k) if norm else None, misalign=misalign)
    out, raw_got, norm_got, rt = ops.gemv_rows(x, w, rows, ys, **kw)
    out2, raw2, norm2, rt2 = ops.gemv_rows(x, w, rows, ys, **kw)
    assert rt == rt2 and all(np.array_equal(bits(a), bits(c)) for a, c in zip(out, out2)), f"{group} {case}: two runs differ"
    assert all(a is None or np.array_equal(bits(a), bits(c)) for a, c in ((raw_got, raw2), (norm_got, norm2)))
    # the route: the launcher's own report against the rule restated, and against the family of the case
    want = W.route(rows, n_out, k, ldx=x.shape[1], seg=seg, epi=epi, gamma=ln, beta=ln or loose_beta, x_raw_out=raw, x_norm_out=norm, misalign=misalign)
    assert rt == want == want_route, (group, case, rt, want, want_route)
    if seg:
        q, kk, v = W.segments(ref, seg)
        check(group, case + " Q", out[0], q)
        check(group, case + " K", out[1], kk, row_off)
        check(group, case + " V", out[2], v, row_off)
    else:
        check(group, case, out[0], ref)
    if norm:
        check(group, case + " x_norm_out", norm_got[None, :], W.layer_norm64(x[:1, :k].astype(F64), gamma, beta, EPS))
    return out


def probe_case(group, case, want_route, *, rows, k, n_out, res=False, inplace=False, seg=0, row_off=0, misalign=0, salt=0, loose_beta=False,
               ldx_pad=4):
    """Exact: row r holds small integers and 1000 at chunk column r of chunk_columns(k) (all of them in turn for one row); integer
    bias and residual.  Every output must equal the integer sum, bit for bit."""
    ops = _ops()
    cols = chunk_columns(k)
    wi = int_mat(n_out, k, salt)
    bi = (np.arange(n_out, dtype=np.int64) * 3) % 11 - 5
    calls = [cols[i:i + rows] for i in range(0, len(cols), rows)]
    for at in calls:
        at = (at + cols)[:rows]
        xi = (np.arange(rows, dtype=np.int64)[:, None] * 3 + np.arange(k, dtype=np.int64)[None, :] * 5) % 7 - 3
        for r_, c in enumerate(at):
            xi[r_, c] = 1000
        ri = (np.arange(rows, dtype=np.int64)[:, None] * 5 + np.arange(n_out, dtype=np.int64)[None, :] * 7) % 13 - 6
        want = xi @ wi.T + bi + (ri if res else 0)
        assert np.abs(want).max() < 2 ** 24 and 7 * (3 * k + 1000) < 2 ** 24
        x = nans(rows + 1, k + ldx_pad)
        x[:rows, :k] = xi.astype(F32)
        y0 = nans(rows + 1, (seg or n_out) + 3)
        ys = [y0] if not seg else [y0, nans(row_off + rows + 1, seg + 1), nans(row_off + rows + 2, seg + 1)]
        if inplace:
            y0[:rows, :n_out] = ri.astype(F32)
        out, _, _, rt = ops.gemv_rows(x, wi.astype(F32), rows, ys, k=k, bias=bi.astype(F32), r=ri.astype(F32) if res and not inplace else None,
                                      r_is_y0=inplace, seg=seg, row_off=row_off, epi=RES if res else BIAS, misalign=misalign,
                                      beta=np.zeros(k, F32) if loose_beta else None)
        assert rt == want_route, (group, case, rt)
        parts = W.segments(want, seg) if seg else (want,)
        for i, (got, exp) in enumerate(zip(out, parts)):
            r0 = row_off if i else 0
            own = np.zeros(got.shape, bool)
            own[r0:r0 + rows, :exp.shape[1]] = True
            assert (bits(got)[~own] == NAN_BITS).all(), f"{group} {case}: an element outside output {i} was written"
            assert np.array_equal(got[r0:r0 + rows, :exp.shape[1]], exp.astype(F32)), f"{group} {case} columns {at}: output {i} is not the integer sum"


# ---- one row of 512 / 2048 floats: gemv_row_fast_kernel ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_out", (1, 4, 5, 7))
@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
@pytest.mark.parametrize("k", (512, 2048))
def test_one_row_fast(k, pair, n_out):
    proj_case("one-row fast", f"k={k} {PNAME[pair]} n={n_out}", W.ONE_FAST, rows=1, k=k, n_out=n_out, pair=pair, pads=(8, 3, 0, 2))


@pytest.mark.parametrize("on_device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("row_off", (0, 3))
@pytest.mark.parametrize("seg", (4, 5))
@pytest.mark.parametrize("k", (512, 2048))
def test_one_row_fast_segments(k, seg, row_off, on_device):
    proj_case("one-row fast", f"k={k} seg={seg} off={row_off} dev={on_device}", W.ONE_FAST, rows=1, k=k, n_out=3 * seg, pair=(BIAS, True),
              seg=seg, row_off=row_off, on_device=on_device, pads=(4, 1, 2, 0))
    if k == 512:
        proj_case("one-row fast", f"k={k} seg={seg} off={row_off} dev={on_device} plain", W.ONE_FAST, rows=1, k=k, n_out=3 * seg,
                  pair=(BIAS, False), seg=seg, row_off=row_off, on_device=on_device, pads=(4, 1, 2, 0))


@pytest.mark.parametrize("k", (512, 2048))
def test_one_row_fast_in_place_residual_and_extras(k):
    proj_case("one-row fast", f"k={k} in place", W.ONE_FAST, rows=1, k=k, n_out=7, pair=(RES, False), inplace=True, pads=(8, 2, 0, 0))
    proj_case("one-row fast", f"k={k} x_norm_out", W.ONE_FAST, rows=1, k=k, n_out=5, pair=(BIAS, True), norm=True)
    proj_case("one-row fast", f"k={k} x_norm_out gelu", W.ONE_FAST, rows=1, k=k, n_out=5, pair=(GELU, True), norm=True)
    proj_case("one-row fast", f"k={k} x_norm_out seg", W.ONE_FAST, rows=1, k=k, n_out=12, pair=(BIAS, True), norm=True, seg=4, row_off=1)


@pytest.mark.parametrize("k", (512, 2048))
def test_one_row_fast_probes(k):
    probe_case("one-row fast", f"k={k}", W.ONE_FAST, rows=1, k=k, n_out=5)
    probe_case("one-row fast", f"k={k} in place", W.ONE_FAST, rows=1, k=k, n_out=6, res=True, inplace=True, salt=1)
    probe_case("one-row fast", f"k={k} seg", W.ONE_FAST, rows=1, k=k, n_out=12, seg=4, row_off=2, salt=2)


# ---- the embed variant ---------------------------------------------------------------------------------------------------------------

VOCAB, MAX_POS = 7, 5


def _tables():
    if "emb" not in _CACHE:
        rng = np.random.default_rng(77)
        _CACHE["emb"] = (rng.standard_normal((VOCAB, 512)).astype(F32) * F32(0.05), rng.standard_normal((MAX_POS, 512)).astype(F32))
    return _CACHE["emb"]


@pytest.mark.parametrize("pos_dev", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("scaled", (False, True), ids=("scale1", "sqrt512"))
@pytest.mark.parametrize("pos", (0, MAX_POS - 1, MAX_POS))
@pytest.mark.parametrize("idx", (0, VOCAB - 1, VOCAB))
def test_embed_variant(idx, pos, scaled, pos_dev):
    """LN + Q | K | V from a row the kernel builds itself: on the bar against float64, and bit-equal to decoder_embed followed by the
    plain one-row call, x_raw_out included."""
    ops = _ops()
    word, pos_t = _tables()
    seg, row_off, k = 4, 2, 512
    scale = float(np.sqrt(F32(512.0))) if scaled else 1.0
    rng = np.random.default_rng([idx, pos, int(scaled)])
    w = mat(3 * seg, k)
    gamma, beta = (1.0 + 0.1 * rng.standard_normal(k)).astype(F32), (0.1 * rng.standard_normal(k)).astype(F32)
    b = (0.1 * rng.standard_normal(3 * seg)).astype(F32)
    ys = [nans(2, seg + 1), nans(6, seg + 2), nans(6, seg + 2)]
    emb = dict(id=idx, word=word, pos_table=pos_t, pos=pos, pos_on_device=pos_dev, scale=scale)
    kw = dict(k=k, gamma=gamma, beta=beta, eps=EPS, bias=b, seg=seg, row_off=row_off, offset_on_device=pos_dev)
    out, raw, _, rt = ops.gemv_rows(None, w, 1, ys, embed=emb, x_raw_out=nans(k), **kw)
    out2, raw2, _, _ = ops.gemv_rows(None, w, 1, ys, embed=emb, x_raw_out=nans(k), **kw)
    assert rt == W.ONE_FAST_EMBED == W.route(1, 3 * seg, k, seg=seg, gamma=True, embed=True, x_raw_out=True)
    assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(out + [raw], out2 + [raw2]))
    case = f"id={idx} pos={pos} {'sqrt512' if scaled else 'scale1'} dev={pos_dev}"
    row64 = W.embed64(word, idx, scale, pos_t, pos)
    check("embed", case + " x_raw_out", raw[None, :], row64[None, :])
    assert np.array_equal(bits(raw), bits(W.embed32(word, idx, scale, pos_t, pos))), case
    if idx >= VOCAB:
        assert np.array_equal(raw, pos_t[pos] if pos < MAX_POS else np.zeros(k, F32)), case
    ref = W.layer_norm64(row64[None, :], gamma, beta, EPS) @ w.astype(F64).T + b.astype(F64)
    for name, got, exp, r0 in zip("QKV", out, W.segments(ref, seg), (0, row_off, row_off)):
        check("embed", f"{case} {name}", got, exp, r0)
    # the two-launch form the variant replaces
    row = ops.decoder_embed([idx], word, pos_t, pos, nans(1, k), offset_on_device=pos_dev, scale_embeddings=scaled)
    assert np.array_equal(bits(row[0]), bits(raw)), f"{case}: x_raw_out is not decoder_embed's row"
    plain, _, _, rt1 = ops.gemv_rows(row, w, 1, ys, **kw)
    assert rt1 == W.ONE_FAST and all(np.array_equal(bits(a), bits(c)) for a, c in zip(out, plain)), f"{case}: not decoder_embed + the one-row call"
    # without x_raw_out and without a position table
    out3, _, _, rt3 = ops.gemv_rows(None, w, 1, ys, embed=emb, **kw)
    assert rt3 == W.ONE_FAST_EMBED and all(np.array_equal(bits(a), bits(c)) for a, c in zip(out, out3))
    if pos == 0 and not pos_dev:
        out4, raw4, _, _ = ops.gemv_rows(None, w, 1, ys, embed=dict(emb, pos_table=None), x_raw_out=nans(k), **kw)
        assert np.array_equal(bits(raw4), bits(W.embed32(word, idx, scale, None, 0)))
        check("embed", case + " no table", out4[0], (W.layer_norm64(raw4[None, :].astype(F64), gamma, beta, EPS) @ w.astype(F64).T + b)[:, :seg])


def test_embed_variant_refusals_write_nothing():
    ops = _ops()
    exc, code = _refused()
    word, pos_t = _tables()
    g, be = np.ones(512, F32), np.zeros(512, F32)
    emb = dict(id=1, word=word, pos_table=pos_t, pos=1)
    for kw in (dict(), dict(gamma=g, beta=be, epi=GELU), dict(gamma=g, beta=be, misalign=4), dict(gamma=g, beta=be, misalign=2),
               dict(epi=RES, r=np.zeros((1, 6), F32))):
        with pytest.raises(exc) as e:
            ops.gemv_rows(None, mat(6, 512), 1, [nans(2, 6)], embed=emb, **kw)
        assert e.value.code == code, kw
    w2k = mat(6, 2048)
    with pytest.raises(exc):
        ops.gemv_rows(None, w2k, 1, [nans(2, 6)], embed=dict(id=1, word=np.zeros((3, 2048), F32), pos=0), gamma=np.ones(2048, F32), beta=np.zeros(2048, F32))


# ---- 2..8 rows of 512 / 2048 floats staged in LDS: gemv_rows_lds_fast_kernel -----------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
@pytest.mark.parametrize("k,rows", [(512, r) for r in range(2, 9)] + [(2048, r) for r in (2, 5, 6, 8)])
def test_staged_fast(k, rows, pair):
    """2048 x 6 rows is the first above 48 KiB of LDS (the dynamic opt-in), 2048 x 8 exactly 64 KiB; rows of very different norms."""
    scales = [1.0, 0.01, 30.0, 1.0, 3.0, 0.1, 1.0, 10.0] if pair[1] else None
    proj_case("staged fast", f"k={k} rows={rows} {PNAME[pair]}", W.STAGED_FAST, rows=rows, k=k, n_out=6, pair=pair, pads=(8, 2, 0, 3), scales=scales)


@pytest.mark.parametrize("n_out", (5, 6, 7))
@pytest.mark.parametrize("k", (512, 2048))
def test_staged_fast_surplus_waves_segments_and_residuals(k, n_out):
    """n_out 5 .. 7: the last workgroup's surplus waves stage rows with the clamped column.  Segments with the row on the device,
    ldr != n_out, the residual in place."""
    for pair in PAIRS:
        proj_case("staged fast", f"k={k} n={n_out} {PNAME[pair]}", W.STAGED_FAST, rows=3, k=k, n_out=n_out, pair=pair, pads=(4, 1, 0, 5))
    proj_case("staged fast", f"k={k} n={n_out} in place", W.STAGED_FAST, rows=5, k=k, n_out=n_out, pair=(RES, False), inplace=True, pads=(4, 3, 0, 0))
    if n_out == 5:
        for row_off, dev in ((0, True), (3, True), (1, False)):
            proj_case("staged fast", f"k={k} seg=5 off={row_off} dev={dev}", W.STAGED_FAST, rows=3, k=k, n_out=15, pair=(BIAS, True), seg=5,
                      row_off=row_off, on_device=dev, pads=(4, 1, 2, 0), cache_rows=7)


@pytest.mark.parametrize("k", (512, 2048))
def test_staged_fast_probes(k):
    probe_case("staged fast", f"k={k}", W.STAGED_FAST, rows=8, k=k, n_out=7)
    probe_case("staged fast", f"k={k} in place", W.STAGED_FAST, rows=5, k=k, n_out=6, res=True, inplace=True, salt=1)
    probe_case("staged fast", f"k={k} residual", W.STAGED_FAST, rows=2, k=k, n_out=5, res=True, salt=3)
    probe_case("staged fast", f"k={k} seg", W.STAGED_FAST, rows=3, k=k, n_out=15, seg=5, row_off=2, salt=2)


# ---- the vocabulary head: gemv_rows_head_kernel ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("n_out", (8192, 8193, 8207))
@pytest.mark.parametrize("rows", (2, 5, 8))
def test_head(rows, n_out, bias):
    """8193 and 8207 leave a workgroup 1 and 15 of its 16 columns: the surplus columns read the clamped weight row and store nothing."""
    proj_case("head", f"rows={rows} n={n_out} bias={bias}", W.HEAD, rows=rows, k=512, n_out=n_out, pair=(BIAS, False), bias=bias,
              pads=(8, 5, 0, 0), w_rows=8207)


def test_head_threshold_and_probes():
    proj_case("staged fast", "rows=2 n=8191 (below the head)", W.STAGED_FAST, rows=2, k=512, n_out=8191, pair=(BIAS, False), w_rows=8207)
    probe_case("head", "n=8193", W.HEAD, rows=8, k=512, n_out=8193)
    probe_case("head", "n=8207 rows=3", W.HEAD, rows=3, k=512, n_out=8207, salt=1)


def test_head_rows_equal_the_one_row_call_bit_for_bit():
    ops = _ops()
    rows, k, n_out = 5, 512, 8193
    x, w, _, _, b, _ = operands(rows, k, n_out, (BIAS, False), w_rows=8207)
    head, _, _, rt = ops.gemv_rows(x, w, rows, [nans(rows, n_out)], k=k, bias=b)
    assert rt == W.HEAD
    for r in range(rows):
        one, _, _, rt1 = ops.gemv_rows(x[r:r + 1], w, 1, [nans(1, n_out)], k=k, bias=b)
        assert rt1 == W.ONE_FAST and np.array_equal(bits(one[0]), bits(head[0][r:r + 1])), r


# ---- 2..8 rows of any width staged in LDS (gemv_rows_lds_kernel) and the general kernel (gemv_rows_kernel) ----------------------------

WIDTHS = (4, 64, 252, 260, 384, 768, 1280)       # 384 / 768 / 1280 (and 1024 below): the tiny, small, large and medium models


@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
@pytest.mark.parametrize("rows", (2, 8))
@pytest.mark.parametrize("k", WIDTHS + (1024,))
def test_staged_general(k, rows, pair):
    proj_case("staged", f"k={k} rows={rows} {PNAME[pair]}", W.STAGED, rows=rows, k=k, n_out=7, pair=pair, pads=(4, 2, 0, 3))


@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
def test_staged_general_at_the_lds_budget_and_off_the_fast_kernel(pair):
    """5120 x 3 rows = 60 KiB stages (above 48 KiB: the opt-in); 512 / 2048 with gamma (or a loose beta) 4 bytes off the fast kernels."""
    proj_case("staged", f"k=5120 rows=3 {PNAME[pair]}", W.STAGED, rows=3, k=5120, n_out=6, pair=pair, pads=(4, 1, 0, 2))
    mis = dict(misalign=W.MIS_GAMMA) if pair[1] else dict(misalign=W.MIS_BETA, loose_beta=True)
    for k in (512, 2048):
        proj_case("staged", f"k={k} rows=5 {PNAME[pair]} misaligned", W.STAGED, rows=5, k=k, n_out=6, pair=pair, pads=(4, 1, 0, 2), **mis)
    if pair[1]:
        proj_case("staged", f"k=512 rows=2 {PNAME[pair]} beta misaligned", W.STAGED, rows=2, k=512, n_out=6, pair=pair, misalign=W.MIS_BETA)


def test_staged_general_segments_and_in_place():
    for k in (384, 768):
        proj_case("staged", f"k={k} seg dev", W.STAGED, rows=4, k=k, n_out=15, pair=(BIAS, True), seg=5, row_off=2, on_device=True, pads=(4, 1, 2, 0),
                  cache_rows=7)
        proj_case("staged", f"k={k} seg host", W.STAGED, rows=2, k=k, n_out=12, pair=(BIAS, True), seg=4, row_off=3, pads=(4, 0, 1, 0))
        proj_case("staged", f"k={k} in place", W.STAGED, rows=8, k=k, n_out=7, pair=(RES, False), inplace=True, pads=(4, 3, 0, 0))
        probe_case("staged", f"k={k}", W.STAGED, rows=8, k=k, n_out=7)
        probe_case("staged", f"k={k} in place", W.STAGED, rows=3, k=k, n_out=6, res=True, inplace=True, salt=1)
        probe_case("staged", f"k={k} seg", W.STAGED, rows=2, k=k, n_out=12, seg=4, row_off=1, salt=2)
    probe_case("staged", "k=512 off the fast kernel", W.STAGED, rows=8, k=512, n_out=7, misalign=W.MIS_BETA, loose_beta=True)


@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
@pytest.mark.parametrize("k", WIDTHS + (1024,))
def test_general_one_row(k, pair):
    proj_case("general", f"k={k} {PNAME[pair]}", W.GENERAL, rows=1, k=k, n_out=7, pair=pair, pads=(4, 2, 0, 3))


@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
def test_general_past_the_lds_budget_and_off_the_fast_kernel(pair):
    """5120 x 4 rows = 80 KiB does not stage; one row of 512 / 2048 with gamma (or a loose beta) misaligned."""
    for rows in (4, 8):
        proj_case("general", f"k=5120 rows={rows} {PNAME[pair]}", W.GENERAL, rows=rows, k=5120, n_out=6, pair=pair, pads=(4, 1, 0, 2))
    mis = dict(misalign=W.MIS_GAMMA) if pair[1] else dict(misalign=W.MIS_BETA, loose_beta=True)
    for k in (512, 2048):
        proj_case("general", f"k={k} {PNAME[pair]} misaligned", W.GENERAL, rows=1, k=k, n_out=6, pair=pair, pads=(4, 1, 0, 2), **mis)


def test_general_segments_in_place_and_probes():
    proj_case("general", "k=768 seg dev", W.GENERAL, rows=1, k=768, n_out=15, pair=(BIAS, True), seg=5, row_off=3, on_device=True, pads=(4, 1, 2, 0))
    proj_case("general", "k=5120 rows=5 seg host", W.GENERAL, rows=5, k=5120, n_out=12, pair=(BIAS, True), seg=4, row_off=1, pads=(4, 0, 1, 0), cache_rows=7)
    proj_case("general", "k=5120 rows=8 in place", W.GENERAL, rows=8, k=5120, n_out=7, pair=(RES, False), inplace=True, pads=(4, 3, 0, 0))
    proj_case("general", "k=384 in place", W.GENERAL, rows=1, k=384, n_out=7, pair=(RES, False), inplace=True, pads=(4, 3, 0, 0))
    for k in (384, 1280):
        probe_case("general", f"k={k}", W.GENERAL, rows=1, k=k, n_out=5)
        probe_case("general", f"k={k} in place", W.GENERAL, rows=1, k=k, n_out=6, res=True, inplace=True, salt=1)
    probe_case("general", "k=5120 rows=8", W.GENERAL, rows=8, k=5120, n_out=7)
    probe_case("general", "k=5120 rows=4 seg", W.GENERAL, rows=4, k=5120, n_out=12, seg=4, row_off=2, salt=2)
    probe_case("general", "k=2048 off the fast kernel", W.GENERAL, rows=1, k=2048, n_out=5, misalign=W.MIS_BETA, loose_beta=True)


# ---- the fall-through to launch_gemm, the refusals, nothing to do ---------------------------------------------------------------------

@pytest.mark.parametrize("pair", ((BIAS, False), (RES, False)), ids=PNAME.get)
def test_gemm_fall_through(pair):
    proj_case("gemm", f"rows=9 {PNAME[pair]}", W.GEMM, rows=9, k=512, n_out=7, pair=pair, pads=(4, 2, 0, 3))
    proj_case("gemm", f"k=510 {PNAME[pair]}", W.GEMM, rows=2, k=510, n_out=7, pair=pair, pads=(2, 2, 0, 3))
    proj_case("gemm", f"k=18 {PNAME[pair]}", W.GEMM, rows=1, k=18, n_out=5, pair=pair, pads=(1, 0, 0, 0))
    proj_case("gemm", f"ldx=514 {PNAME[pair]}", W.GEMM, rows=2, k=512, n_out=7, pair=pair, pads=(2, 0, 0, 0))
    proj_case("gemm", f"x misaligned {PNAME[pair]}", W.GEMM, rows=2, k=512, n_out=7, pair=pair, misalign=W.MIS_X)
    proj_case("gemm", f"w misaligned {PNAME[pair]}", W.GEMM, rows=1, k=2048, n_out=7, pair=pair, misalign=W.MIS_W)
    if pair[0] == RES:
        proj_case("gemm", "rows=9 in place", W.GEMM, rows=9, k=384, n_out=7, pair=pair, inplace=True, pads=(4, 3, 0, 0))
    probe_case("gemm", f"rows=9 {PNAME[pair]}", W.GEMM, rows=9, k=512, n_out=7, res=pair[0] == RES)
    probe_case("gemm", f"w misaligned {PNAME[pair]}", W.GEMM, rows=2, k=512, n_out=5, res=pair[0] == RES, misalign=W.MIS_W, salt=1)


def _refusal(**kw):
    """A refused call: INVALID_CONFIG, and (the hook uploads nothing before the rule is asked) nothing to have been written."""
    ops = _ops()
    exc, code = _refused()
    rows, k, n_out = kw.pop("rows", 2), kw.pop("k", 512), kw.pop("n_out", 6)
    seg = kw.get("seg", 0)
    ys = [nans(rows + 1, seg or n_out)] + ([nans(rows + 2, seg), nans(rows + 2, seg)] if seg else [])
    with pytest.raises(exc) as e:
        ops.gemv_rows(nans(rows, kw.pop("ldx", k)), mat(n_out, k), rows, ys, k=k, **kw)
    assert e.value.code == code, kw


def test_refusals():
    g, be = np.ones(512, F32), np.zeros(512, F32)
    r = np.zeros((9, 6), F32)
    ln = dict(gamma=g, beta=be)
    # the GEMM route takes neither gamma nor segments
    for kw in (dict(rows=9, **ln), dict(rows=9, seg=2), dict(k=510, ldx=512, gamma=g[:510], beta=be[:510]), dict(k=510, ldx=512, seg=2),
               dict(misalign=W.MIS_X, **ln), dict(misalign=W.MIS_W, seg=2), dict(ldx=514, **ln)):
        _refusal(**kw)
    # every (epilogue, LayerNorm) pair outside the four, on every route
    for rows, k in ((1, 512), (2, 512), (2, 384), (1, 384), (9, 512)):
        lnk = dict(gamma=np.ones(k, F32), beta=np.zeros(k, F32))
        for kw in (dict(epi=GELU), dict(epi=RES, r=r, **lnk), dict(epi=2), dict(epi=3), dict(epi=4), dict(epi=6, r=r), dict(epi=2, **lnk), dict(epi=6, r=r, **lnk)):
            _refusal(rows=rows, k=k, **kw)
    # the extras outside gemv_rows_takes_row_extras, and where no kernel would write them (x_raw_out belongs to the embed variant:
    # the one-row kernel took it without the embedding and never stored it)
    ln768 = dict(gamma=np.ones(768, F32), beta=np.zeros(768, F32))
    for kw in (dict(rows=2, x_norm_out=nans(512), **ln), dict(rows=1, k=768, x_norm_out=nans(768), **ln768), dict(rows=1, x_norm_out=nans(512)),
               dict(rows=1, x_norm_out=nans(512), misalign=W.MIS_GAMMA, **ln), dict(rows=1, x_norm_out=nans(512), misalign=W.MIS_X, **ln),
               dict(rows=1, x_norm_out=nans(512), misalign=W.MIS_W, **ln), dict(rows=1, x_raw_out=nans(512)), dict(rows=1, x_raw_out=nans(512), **ln),
               dict(rows=1, x_raw_out=nans(512), epi=RES, r=r)):
        _refusal(**kw)
    # arguments a kernel would have followed out of its buffers
    for kw in (dict(gamma=g), dict(rows=1, gamma=g), dict(epi=RES), dict(rows=1, epi=RES), dict(seg=1), dict(rows=1, seg=1, n_out=4)):
        _refusal(**kw)


@pytest.mark.parametrize("rows,n_out", ((0, 6), (-1, 6), (2, 0), (2, -1)))
def test_nothing_to_do_writes_nothing(rows, n_out):
    ops = _ops()
    for k, kw in ((512, {}), (384, dict(gamma=np.ones(384, F32), beta=np.zeros(384, F32))), (510, {})):
        out, raw, nrm, rt = ops.gemv_rows(nans(2, k), mat(6, k), rows, [nans(3, 6)], k=k, n_out=n_out, **kw)
        assert rt == W.NOTHING == W.route(rows, n_out, k, gamma=bool(kw))
        untouched("nothing", f"rows={rows} n={n_out} k={k}", out[0])


# ---- bit identity: a row's result whichever kernel computes it ------------------------------------------------------------------------

@pytest.mark.parametrize("pair", PAIRS, ids=PNAME.get)
@pytest.mark.parametrize("k", (512, 2048, 768))
def test_a_row_is_the_same_bits_whichever_kernel_computes_it(k, pair):
    """Row r of an 8-row call (staged fast at 512 / 2048, staged at 768) = the one-row call on that row (one-row fast; general at 768)
    = the general and the staged kernels reached by misaligning gamma (without LayerNorm: a loose beta)."""
    ops = _ops()
    epi, ln = pair
    rows, n_out = 8, 9
    scales = [1.0, 0.01, 30.0, 1.0, 3.0, 0.1, 1.0, 10.0] if ln else None
    x, w, gamma, beta, b, r = operands(rows, k, n_out, pair, seed=5, pads=(0, 0, 0, 0), scales=scales)
    x = x[:rows]
    kw = dict(k=k, gamma=gamma, beta=beta, eps=EPS, bias=b, epi=epi)
    mis = dict(misalign=W.MIS_GAMMA) if ln else dict(misalign=W.MIS_BETA, beta=np.zeros(k, F32))
    wide = k in (512, 2048)
    all8, _, _, rt = ops.gemv_rows(x, w, rows, [nans(rows, n_out)], r=r, **kw)
    assert rt == (W.STAGED_FAST if wide else W.STAGED)
    check("bit identity", f"k={k} {PNAME[pair]}", all8[0], W.gemv_rows64(x, w, gamma=gamma, beta=beta, eps=EPS, bias=b, epi=epi, r=r))
    if wide:
        staged, _, _, rt = ops.gemv_rows(x, w, rows, [nans(rows, n_out)], r=r, **dict(kw, **mis))
        assert rt == W.STAGED and np.array_equal(bits(staged[0]), bits(all8[0])), "staged != staged fast"
    for i in range(rows):
        ri = None if r is None else r[i:i + 1]
        one, _, _, rt = ops.gemv_rows(x[i:i + 1], w, 1, [nans(1, n_out)], r=ri, **kw)
        assert rt == (W.ONE_FAST if wide else W.GENERAL) and np.array_equal(bits(one[0]), bits(all8[0][i:i + 1])), f"row {i}: one-row call differs"
        if wide:
            gen, _, _, rt = ops.gemv_rows(x[i:i + 1], w, 1, [nans(1, n_out)], r=ri, **dict(kw, **mis))
            assert rt == W.GENERAL and np.array_equal(bits(gen[0]), bits(all8[0][i:i + 1])), f"row {i}: general kernel differs"
    few, _, _, rt = ops.gemv_rows(x[3:], w, 5, [nans(5, n_out)], r=None if r is None else r[3:], **kw)       # the same rows in a call of 5
    assert np.array_equal(bits(few[0]), bits(all8[0][3:]))


# ---- LayerNorm edges ---------------------------------------------------------------------------------------------------------------------

LN_ROUTES = ((1, 512, W.ONE_FAST), (4, 512, W.STAGED_FAST), (1, 2048, W.ONE_FAST), (3, 384, W.STAGED), (1, 384, W.GENERAL), (1, 768, W.GENERAL))


@pytest.mark.parametrize("rows,k,want", LN_ROUTES)
@pytest.mark.parametrize("epi", (BIAS, GELU), ids=("bias", "gelu"))
def test_layernorm_edges(rows, k, want, epi):
    ops = _ops()
    rng = np.random.default_rng([rows, k, epi])
    group = "layernorm edges"
    # a constant row: variance 0, the normalised row is beta exactly, the result beta . W + bias -- the plain call on beta, bit for bit
    x = np.full((rows, k), 3.0, F64)
    out = proj_case(group, f"constant rows={rows} k={k} epi={epi}", want, rows=rows, k=k, n_out=7, pair=(epi, True), x_values=x, pads=(4, 1, 0, 0))
    if epi == BIAS:
        _, w, _, beta, b, _ = operands(rows, k, 7, (epi, True), pads=(4, 1, 0, 0), x_values=x)
        plain, _, _, _ = ops.gemv_rows(np.tile(beta, (rows, 1)), w, rows, [nans(rows, 7)], k=k, bias=b)
        assert np.array_equal(bits(plain[0]), bits(out[0][:rows, :7])), "a constant row is not beta . W + bias"
    # mean square 1e-4: eps = 1e-5 is a tenth of the variance and moves the result by 5 %
    small = 0.01 * rng.standard_normal((rows, k))
    proj_case(group, f"small rows={rows} k={k} epi={epi}", want, rows=rows, k=k, n_out=7, pair=(epi, True), x_values=small, pads=(4, 1, 0, 0))
    _, w, gamma, beta, b, _ = operands(rows, k, 7, (epi, True), pads=(4, 1, 0, 0), x_values=small)
    with_eps = W.gemv_rows64(small.astype(F32), w, gamma=gamma, beta=beta, eps=EPS, bias=b, epi=epi)
    assert np.abs(with_eps - W.gemv_rows64(small.astype(F32), w, gamma=gamma, beta=beta, eps=0.0, bias=b, epi=epi)).max() > 10 * W.bar(with_eps)
    # a large mean, the noise in sixteenths (the module's docstring) and summing to zero: exact sums and a mean of exactly 1000 at
    # every k, so only a one-pass variance fails
    q = 16.0 if k <= 512 else 4.0
    noise = np.round(rng.standard_normal((rows, k)) * q) / q
    noise[:, -1] -= noise.sum(axis=1)
    large = 1000.0 + noise
    assert (large.mean(axis=1) == 1000.0).all()
    assert float(np.abs(large).max()) * k * q < 2 ** 24
    proj_case(group, f"large mean rows={rows} k={k} epi={epi}", want, rows=rows, k=k, n_out=7, pair=(epi, True), x_values=large, pads=(4, 1, 0, 0))


# ---- the front end, bit for bit ---------------------------------------------------------------------------------------------------------

def hann(n):
    i = np.arange(n, dtype=F64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / n))).astype(F32)


def same_bits(what, got, want):
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} elements differ"


@pytest.mark.parametrize("n", (1, 2, 199, 200, 201, 800, 1000))
def test_mel_frames(n):
    """n_fft 400, hop 160, ld 512, 8 frames: the padded signal is n + 400 long, so 1 .. 201 samples give one or two live frames, 800
    six and 1000 seven -- the rest lie past the padded end and are zero, as are columns 400 .. 511."""
    ops = _ops()
    audio = np.random.default_rng(n).standard_normal(n).astype(F32)
    win = hann(400) + F32(0.25)            # (no zero in the window: a sample taken from the wrong place shows at every column)
    got = ops.mel_frames(audio, win, 160, nans(8, 512))
    ref = W.mel_frames64(audio, win, 160, 8, 512)
    same_bits(f"mel_frames n={n}", got, ref.astype(F32))
    live = sum(1 for f in range(8) if f * 160 + 400 <= n + 400)
    assert live == {1: 1, 2: 1, 199: 2, 200: 2, 201: 2, 800: 6, 1000: 7}[n] and not got[live:].any() and not got[:, 400:].any()
    assert np.abs(got[:live, :400]).min() > 0.0
    same_bits("mel_frames twice", ops.mel_frames(audio, win, 160, nans(8, 512)), got)


def test_mel_frames_ramp_shows_every_reflection():
    """A ramp 1, 2, 3, ... and a window of ones: frame 0 is the padded signal itself."""
    ops = _ops()
    for n in (1, 2, 3, 5, 8, 9, 40):
        audio = np.arange(1, n + 1, dtype=F32)
        got = ops.mel_frames(audio, np.ones(8, F32), 1, nans(n + 3, 12))
        padded = W.pad_reflect(audio, 4)
        assert len(padded) == n + 8
        for f in range(n + 3):
            want = np.zeros(12, F32)
            if f + 8 <= len(padded):
                want[:8] = padded[f:f + 8]
            same_bits(f"ramp n={n} frame {f}", got[f], want)


def test_mel_power():
    ops = _ops()
    rng = np.random.default_rng(9)
    dft = nans(3, 512)
    dft[:, :201] = (rng.standard_normal((3, 201)) * 10.0).astype(F32)
    dft[:, 256:457] = (rng.standard_normal((3, 201)) * 10.0).astype(F32)
    dft[0, 0], dft[0, 256] = 3.0, 4.0
    got = ops.mel_power(dft, 256, 201, nans(3, 208))
    same_bits("mel_power", got, W.mel_power32(dft, 256, 201, 208))
    assert got[0, 0] == 25.0 and not got[:, 201:].any()
    ref = W.mel_power64(dft, 256, 201, 208)
    err = float(np.abs(got - ref).max())
    assert report("whisper_proj mel_power: err / bar", err / W.bar(ref), 1.0) <= 1.0


@pytest.mark.parametrize("t_in,C,stride,pad,t_out,ld_cols", ((5, 3, 1, 1, 5, 12), (6, 4, 2, 1, 3, 16), (7, 80, 2, 1, 4, 256)))
def test_im2col3(t_in, C, stride, pad, t_out, ld_cols):
    ops = _ops()
    x = nans(t_in, C + 3)
    x[:, :C] = np.arange(1, t_in * C + 1, dtype=F32).reshape(t_in, C)
    got = ops.im2col3(x, C, stride, pad, nans(t_out, ld_cols))
    same_bits(f"im2col3 {t_in, C, stride, pad, t_out, ld_cols}", got, W.im2col3_64(x, C, stride, pad, t_out, ld_cols))
    assert not got[0, :C].any() and got[0, C] == 1.0 and not got[:, 3 * C:].any()          # the left padding row, the zero columns


@pytest.mark.parametrize("period,table_rows", ((7, 7), (3, 2), (7, 4)))
def test_add_rows(period, table_rows):
    """The table holds one row more than the call may use (1000s): a row index one too far shows."""
    ops = _ops()
    rng = np.random.default_rng(period)
    x = rng.standard_normal((7, 5)).astype(F32)
    table = np.full((table_rows + 1, 5), 1000.0, F32)
    table[:table_rows] = rng.standard_normal((table_rows, 5)).astype(F32)
    got = ops.add_rows(x, period, table, table_rows)
    same_bits(f"add_rows {period, table_rows}", got, W.add_rows32(x, period, table, table_rows))
    assert np.abs(got).max() < 100.0


@pytest.mark.parametrize("hidden", (5, 64, 300))
def test_decoder_embed(hidden):
    ops = _ops()
    rng = np.random.default_rng(hidden)
    vocab, max_pos = 6, 4
    word, pos = rng.standard_normal((vocab, hidden)).astype(F32), rng.standard_normal((max_pos, hidden)).astype(F32)
    ids = [0, vocab - 1, vocab, 2]
    for scaled in (False, True):
        for dev in (False, True):
            for offset in (0, max_pos - 2, max_pos - 1, max_pos):        # rows run from `offset`: the last ones pass the table's end
                got = ops.decoder_embed(ids, word, pos, offset, nans(4, hidden), offset_on_device=dev, scale_embeddings=scaled)
                same_bits(f"decoder_embed h={hidden} off={offset} dev={dev} scaled={scaled}", got, W.decoder_embed32(ids, word, pos, offset, scaled, False))
                got = ops.decoder_embed(ids, word, pos, offset, nans(4, hidden), offset_on_device=dev, scale_embeddings=scaled, lanes=True)
                same_bits(f"decoder_embed lanes h={hidden} off={offset} dev={dev}", got, W.decoder_embed32(ids, word, pos, offset, scaled, True))
        got = ops.decoder_embed(ids, word, None, 1, nans(4, hidden), scale_embeddings=scaled)
        same_bits("decoder_embed without positions", got, W.decoder_embed32(ids, word, None, 1, scaled, False))
    assert not ops.decoder_embed([vocab], word, pos, max_pos, nans(1, hidden)).any()
    ref64 = np.stack([W.embed64(word, i, float(np.sqrt(F32(hidden))), pos, 1 + s) for s, i in enumerate(ids)])
    got = ops.decoder_embed(ids, word, pos, 1, nans(4, hidden), scale_embeddings=True)
    assert report("whisper_proj decoder_embed: err / bar", float(np.abs(got - ref64).max()) / W.bar(ref64), 1.0) <= 1.0


# ---- the front end against float64: log10, the global maximum, the clamp ----------------------------------------------------------------

def log_case(case, mel, n_mels, ld_out):
    ops = _ops()
    frames = mel.shape[0]
    lg, out = ops.mel_log_normalize(mel, n_mels, nans(frames, ld_out))
    lg2, out2 = ops.mel_log_normalize(mel, n_mels, nans(frames, ld_out))
    assert np.array_equal(bits(lg), bits(lg2)) and np.array_equal(bits(out), bits(out2)), f"{case}: two runs differ"
    ref_lg, ref_out = W.mel_log_normalize64(mel, n_mels)
    assert np.array_equal(bits(lg[:, n_mels:]), bits(mel[:, n_mels:])), f"{case}: a padding column of mel was written"
    check("mel_log_normalize", case + " log", lg[:, :n_mels], ref_lg)
    check("mel_log_normalize", case + " out", out, ref_out)
    return ref_lg, ref_out, out


def energies(frames, n_mels, ld, lo=-3.0, hi=1.0, seed=0):
    """Mel energies 10^U(lo, hi) in the first n_mels columns, the NaN pattern in the padding."""
    rng = np.random.default_rng([frames, n_mels, seed])
    mel = nans(frames, ld)
    mel[:, :n_mels] = (10.0 ** rng.uniform(lo, hi, (frames, n_mels))).astype(F32)
    return mel


@pytest.mark.parametrize("n_mels,ld,ld_out", ((80, 96, 88), (128, 136, 128)))
@pytest.mark.parametrize("frames", (1, 7, 3300))
def test_mel_log_normalize(frames, n_mels, ld, ld_out):
    """3 300 frames of 80 mels are 1 032 blocks of 256: past the 1 024 the maximum's grid holds, so its grid-stride loop runs."""
    assert (3300 * 80 + 255) // 256 > 1024
    mel = energies(frames, n_mels, ld)
    log_case(f"frames={frames} mels={n_mels}", mel, n_mels, ld_out)
    for where in ((0, 0), (frames - 1, n_mels - 1)):                    # the maximum at the first and at the last element
        for lo, active in ((-9.5, True), (-3.0, False)):                # the rest within 12.5 decades of it (clamped), or within 6
            m = energies(frames, n_mels, ld, lo=lo, hi=1.0, seed=1)
            m[where] = 1000.0
            ref_lg, ref_out, out = log_case(f"frames={frames} mels={n_mels} max at {where} clamp={active}", m, n_mels, ld_out)
            clamped = ref_lg < ref_lg.max() - 8.0 - 1e-3
            assert abs(ref_lg.max() - 3.0) < 1e-12 and ref_lg[where] == ref_lg.max() and bool(clamped.any()) == active
            if active:          # every clamped element is the same number, (max - 8 + 4) / 4
                assert len(np.unique(bits(out[:, :n_mels][clamped]))) == 1 and abs(float(out[:, :n_mels][clamped][0]) + 0.25) < 1e-5


@pytest.mark.parametrize("frames", (1, 5, 3300))
def test_mel_log_normalize_when_every_log_is_negative(frames):
    """Everything at or below 1e-10 (zeros and negatives included): every log is -10, the maximum is -10 and out is -1.5 everywhere
    -- the order-preserving encoding of a negative maximum decides it.  Then logs of -9 .. -1: the maximum is the one nearest zero."""
    mel = nans(frames, 88)
    rng = np.random.default_rng(frames)
    mel[:, :80] = (rng.uniform(-1.0, 1.0, (frames, 80)) * 1e-10).astype(F32)
    mel[0, 0], mel[-1, 79] = 0.0, 1e-10
    _, ref_out, out = log_case(f"all floor frames={frames}", mel, 80, 80)
    assert np.abs(ref_out + 1.5).max() < 1e-8 and np.abs(out + 1.5).max() < 1e-5
    m = energies(frames, 80, 88, lo=-9.0, hi=-1.0)
    ref_lg, _, _ = log_case(f"all negative frames={frames}", m, 80, 80)
    assert ref_lg.max() < 0.0


def test_worst_cases_are_reported():
    """(runs last in the file: the largest err / bar of every family, for the log)"""
    for group, (ratio, err, bar, case) in sorted(WORST.items()):
        print(f"[whisper_proj] worst {group}: {ratio:.3f} of the bar (err {err:.3e}, bar {bar:.3e}) at {case}")
