"""The dense (f32 / bf16) decode-step projections alone, kernel by kernel: launch_llm_gemv (llm_gemv_stream_kernel,
llm_gemv_splitk_kernel, llm_gemv1_kernel, llm_gemv_kernel), launch_llm_gemv_lanes (llm_gemv_lanes_kernel) and launch_llm_qkv_rope
(llm_qkv_rope_kernel, llm_qkv_rope_stream_kernel) through kjarni_hip_op_llm_gemv / _llm_qkv_rope, one launch per case, against
tests/dense_proj_ref64.py at the widths and forms the whole-model fixtures never reach.

Every case
  * holds the route the launcher reports (llm_gemv_route / llm_gemv_lanes_route / llm_qkv_rope_route, the functions the launchers
    themselves call) against the Python restatement of the rule and against the kernel family the case is filed under, so a case
    that stops reaching its kernel fails;
  * pre-fills its outputs, the padding columns of x and the rows of x past `rows` with one NaN bit pattern and asserts that every
    element the operation owns is finite and on the bar and that every other element still holds that pattern;
  * runs twice and asserts the same bits.
The probes are exact: integer weights, an integer input row whose squares sum to K (so RMSNorm with eps = 0 and gamma = 1 divides by
exactly 1), its largest entry at the first or last element of a piece, chunk or slice; every sum is an integer below 2^24, so any
order of summation gives the same f32 and a weight or an input element taken from the wrong place gives another integer.

The bar: 1e-5 x max(1, max |ref|) against float64, the bar of test_gpu_quant_proj / test_gpu_gguf / test_gpu_fp8 for these kernels,
at every K up to 16 392.  Inputs are scaled so that max |ref| stays O(1 - 10) (the saturated SwiGLU gates apart)."""
import math

import numpy as np
import pytest

from tests import dense_proj_ref64 as D
from tests.parity_report import report

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN_BITS = np.uint32(0x7FC01234)
DT = (False, True)                                   # bf16
DNAME = {False: "f32", True: "bf16"}
FORMS = ("plain", "rms", "swiglu", "residual", "inplace")
LN_FORMS = ("ln", "ln+gelu")
EPS = 1e-5
SMALL = (0.01,)          # a row of mean square 1e-4: eps = 1e-5 moves its RMSNorm by 5 %, a norm without eps is off the bar


def _ops():
    from kjarni_amd import ops
    return ops


def nans(*shape):
    return np.full(shape, NAN_BITS, np.uint32).view(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- operands, made once -------------------------------------------------------------------------------------------------------------

_CACHE = {}


def mat(n, k, bf16, seed=0):
    """Weights [n, k] ~ N(0, 1 / k) in the dtype the entry takes (f32, or bf16 bit patterns), shared and never changed; a case that
    needs fewer rows slices the first ones."""
    key = ("w", n, k, bf16, seed)
    if key not in _CACHE:
        w = np.random.default_rng([n, k, seed]).standard_normal((n, k), dtype=F32) * F32(1.0 / math.sqrt(k))
        _CACHE[key] = _ops().to_bf16(w) if bf16 else w
    return _CACHE[key]


def int_mat(n, k, bf16, salt=0):
    """Integer weights in -7 .. 7 (exact in either dtype), no two neighbouring rows or columns alike."""
    key = ("i", n, k, bf16, salt)
    if key not in _CACHE:
        r, c = np.arange(n, dtype=np.int64)[:, None], np.arange(k, dtype=np.int64)[None, :]
        w = ((r * 31 + c * 17 + (r * c) % 7 + c // 64 + salt * 5) % 15 - 7).astype(F32)
        _CACHE[key] = (_ops().to_bf16(w) if bf16 else w, w.astype(np.int64))
    return _CACHE[key]


def four_squares(k):
    """k = a^2 + b^2 + c^2 + d^2 with a >= b >= c >= d >= 0 (Lagrange), the first found from the largest a down."""
    key = ("sq", k)
    if key not in _CACHE:
        for a in range(math.isqrt(k), 0, -1):
            for b in range(min(a, math.isqrt(k - a * a)), -1, -1):
                r2 = k - a * a - b * b
                for c in range(min(b, math.isqrt(r2)), -1, -1):
                    d = math.isqrt(r2 - c * c)
                    if d <= c and d * d == r2 - c * c:
                        _CACHE[key] = (a, b, c, d)
                        break
                if key in _CACHE:
                    break
            if key in _CACHE:
                break
    return _CACHE[key]


def probe_row(k, j):
    """An integer row with squares summing to k: the largest entry at column j, the others at three fixed helper columns."""
    x = np.zeros(k, np.int64)
    a, b, c, d = four_squares(k)
    x[j] = a
    helpers = [h for h in (k // 3 + 1, (2 * k) // 3 + 2, k // 7 + 3, 5, 4, 2) if h != j and h < k][:3]
    for h, v in zip(helpers, (b, c, d)):
        x[h] = -v if h % 2 else v
    assert int((x * x).sum()) == k
    return x


def gamma_of(rng, k):
    return (1.0 + 0.1 * rng.standard_normal(k)).astype(F32)


def make_x(rng, rows, k, ldx_pad=8, extra_rows=1, scales=None):
    """x [rows + extra_rows, k + ldx_pad]: normal rows (of the given scales) in [:rows, :k], the NaN pattern everywhere else."""
    x = nans(rows + extra_rows, k + ldx_pad)
    v = rng.standard_normal((rows, k))
    if scales is not None:
        v = v * np.asarray(scales, F64)[:rows, None]
    x[:rows, :k] = v.astype(F32)
    return x


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
    err, bar = float(np.abs(val - ref).max()), D.bar(ref)
    ratio = err / bar
    if ratio >= WORST.get(group, (0.0,))[0]:
        WORST[group] = (ratio, err, bar, case)
    print(f"[dense_proj] {group} {case}: err {err:.3e} bar {bar:.3e} ({ratio:.2f} of it)")
    report(f"dense_proj {group}: largest err / bar", ratio, 1.0)
    assert err <= bar, f"{group} {case}: err {err:.3e} > bar {bar:.3e}"


def untouched(group, case, a):
    assert (bits(a) == NAN_BITS).all(), f"{group} {case}: an array the call does not own was written"


# ---- one launch of launch_llm_gemv / launch_llm_gemv_lanes ---------------------------------------------------------------------------

def gemv_case(group, case, kernel, *, rows, k, n_out, bf16, form, lanes=False, bias=True, seg=None, row_off=0, on_device=False,
              norm_out=False, pads=(8, 0, 0, 0), cache_rows=6, scales=None, seed=0, w_rows=None, gate=None):
    """form: plain | rms | swiglu | residual | inplace | ln | ln+gelu.  seg = (seg_q, seg_kv).  pads = (ldx - k, ldy0 - columns,
    ldy12 - seg_kv, ldr - n_out).  kernel: the family the case is filed under (lanes: whether the lanes kernel takes it).
    gate: +-g puts the SwiGLU gate sums of all columns at +-g (alternating)."""
    ops = _ops()
    rng = np.random.default_rng([seed, rows, k, n_out, int(bf16), len(form)])
    swiglu, ln, res = form == "swiglu", form in LN_FORMS, form in ("residual", "inplace")
    if form in ("plain", "residual", "inplace"):
        scales = None          # (no norm: the scales would only widen the bar of the small rows)
    x = make_x(rng, rows, k, pads[0], scales=scales)
    w = mat(w_rows or n_out, k, bf16)[:n_out]
    w2 = mat(w_rows or n_out, k, bf16, seed=1)[:n_out] if swiglu else None
    gamma = gamma_of(rng, k) if form in ("rms", "swiglu") or ln else None
    beta = (0.1 * rng.standard_normal(k)).astype(F32) if ln else None
    b = (0.1 * rng.standard_normal(n_out)).astype(F32) if bias else None
    if gate is not None:           # w row n = +-gate * xn / |xn|^2: the gate sum is +-gate (to the weights' rounding)
        xn = D.rms_norm64(x[:1, :k].astype(F64), gamma, EPS)[0]
        sign = np.where(np.arange(n_out) % 2 == 0, 1.0, -1.0)[:, None]
        w = (sign * gate * xn[None, :] / float(xn @ xn)).astype(F32)
        w, b = (ops.to_bf16(w) if bf16 else w), None
    r = rng.standard_normal((rows, n_out + pads[3])).astype(F32) if res else None
    ref = D.gemv64(x[:rows, :k], w, gamma=gamma, beta=beta, eps=EPS, layernorm=ln, gelu_tanh=form == "ln+gelu", w2=w2, swiglu=swiglu,
                   bias=b, r=None if r is None else r[:, :n_out], bf16=bf16)
    seg_q, seg_kv = seg or (0, 0)
    y0 = nans(rows + 1, (seg_q or n_out) + pads[1])
    ys = [y0] if not seg else [y0, nans(cache_rows, seg_kv + pads[2]), nans(cache_rows, seg_kv + pads[2])]
    if form == "inplace":
        y0[:rows, :n_out] = r[:, :n_out]
    no = nans(k) if norm_out else None
    kw = dict(lanes=lanes, gamma=gamma, beta=beta, eps=EPS, layernorm=ln, gelu_tanh=form == "ln+gelu", w2=w2, bf16=bf16, swiglu=swiglu, bias=b,
              r=r if form == "residual" else None, r_is_y0=form == "inplace", seg_q=seg_q, seg_kv=seg_kv, row_off=row_off,
              offset_on_device=on_device, norm_out=no)
    out, no_got, rt = ops.llm_gemv(x, w, rows, ys, k=k, **kw)
    out2, no2, rt2 = ops.llm_gemv(x, w, rows, ys, k=k, **kw)
    assert rt == rt2 and all(np.array_equal(bits(a), bits(c)) for a, c in zip(out, out2)), f"{group} {case}: two runs differ"
    assert no is None or np.array_equal(bits(no_got), bits(no2))
    # the route: the launcher's own report against the rule restated, and against the family of the case
    want = D.gemv_route(rows, k, n_out, bf16=bf16, norm=gamma is not None, layernorm=ln, gelu_tanh=form == "ln+gelu", swiglu=swiglu, seg_q=seg_q)
    if lanes:
        lw = D.lanes_route(rows, k, n_out, bf16=bf16, swiglu=swiglu, norm_out=norm_out)
        assert {f: rt[f] for f in lw} == lw and rt["streamed"] == lw["taken"] == int(kernel), (case, rt, lw)
        assert lw["taken"] or rt["fallback"] == want, (case, rt, want)
    else:
        assert rt == want and rt["kernel"] == kernel, (case, rt, want)
    if seg:
        q, kk, v = D.segments(ref, seg_q, seg_kv)
        check(group, case + " Q", out[0], q)
        check(group, case + " K", out[1], kk, row_off)
        check(group, case + " V", out[2], v, row_off)
    else:
        check(group, case, out[0], ref)
    if norm_out:
        xn = D.rms_norm64(x[:1, :k].astype(F64), gamma, EPS)
        check(group, case + " norm_out", no_got[None, :], xn)
    return rt


def probe_case(group, case, kernel, *, rows, k, n_out, bf16, form, cols, lanes=False, seg=None, row_off=0, salt=0):
    """Exact: row r is probe_row(k, cols[r]); plain, rms (eps 0, gamma 1: a division by exactly 1), residual or inplace with integer
    bias and residual.  Every output must equal the integer sum, bit for bit."""
    ops = _ops()
    w, wi = int_mat(n_out, k, bf16, salt)
    xi = np.stack([probe_row(k, j) for j in cols])
    x = nans(rows + 1, k + 4)
    x[:rows, :k] = xi.astype(F32)
    bi = (np.arange(n_out, dtype=np.int64) * 3) % 11 - 5
    ri = ((np.arange(rows, dtype=np.int64)[:, None] * 5 + np.arange(n_out, dtype=np.int64)[None, :] * 7) % 13 - 6)
    res = form in ("residual", "inplace")
    want = xi @ wi.T + bi + (ri if res else 0)
    seg_q, seg_kv = seg or (0, 0)
    y0 = nans(rows + 1, (seg_q or n_out) + 3)
    ys = [y0] if not seg else [y0, nans(row_off + rows + 1, seg_kv + 1), nans(row_off + rows + 2, seg_kv + 1)]
    if form == "inplace":
        y0[:rows, :n_out] = ri.astype(F32)
    out, _, rt = ops.llm_gemv(x, w, rows, ys, k=k, lanes=lanes, gamma=np.ones(k, F32) if form == "rms" else None, eps=0.0, bf16=bf16,
                              bias=bi.astype(F32), r=ri.astype(F32) if form == "residual" else None, r_is_y0=form == "inplace", seg_q=seg_q,
                              seg_kv=seg_kv, row_off=row_off)
    if lanes:
        assert rt["streamed"] == int(kernel), (case, rt)
    else:
        assert rt["kernel"] == kernel, (case, rt)
    parts = D.segments(want, seg_q, seg_kv) if seg else [want]
    for i, (got, ref) in enumerate(zip(out, parts)):
        r0 = row_off if i else 0
        own = np.zeros(got.shape, bool)
        own[r0:r0 + rows, :ref.shape[1]] = True
        assert (bits(got)[~own] == NAN_BITS).all(), f"{group} {case}: an element outside output {i} was written"
        val = got[r0:r0 + rows, :ref.shape[1]]
        bad = np.argwhere(val != ref.astype(F32))
        assert bad.size == 0, f"{group} {case} columns {list(cols)}: output {i} differs first at (row, column) {bad[0]}: {val[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


def edges(k, step):
    """The first and last column of every `step`-wide part of K, and of the 8-column pieces at either end."""
    pos = {0, 7, 8, k - 8, k - 1}
    for s in range(0, k, step):
        pos |= {s, min(s + step, k) - 1}
    return sorted(p for p in pos if 0 <= p < k)


# ---- 1. launch_llm_gemv, one row, the weight-streaming kernel (K = 2048 / 4096 / 8192) -----------------------------------------------

STREAM_K = (2048, 4096, 8192)


@pytest.mark.parametrize("bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_stream_every_pair(k, bf16, form, bias):
    gemv_case("stream", f"{DNAME[bf16]} K={k} {form} bias={int(bias)}", D.STREAM, rows=1, k=k, n_out=5, bf16=bf16, form=form, bias=bias,
              scales=None if bias else SMALL)


@pytest.mark.parametrize("n_out", (1, 5, 1027))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_stream_narrow_form(k, bf16, n_out):
    rt = gemv_case("stream", f"{DNAME[bf16]} K={k} n={n_out} rms", D.STREAM, rows=1, k=k, n_out=n_out, bf16=bf16, form="rms", w_rows=1027)
    assert (rt["wide"], rt["loop"], rt["threads"], rt["rows_per_batch"], rt["workgroups"]) == (0, 0, 256, 1, (n_out + 3) // 4)


@pytest.mark.parametrize("bf16,form,n_out,wide,loop,rpb,wgs", [
    (True, "plain", 8191, 1, 1, 4, 512),      # 8 191 one-row batches are past the 4 096 a grid takes: the looping form already
    (True, "plain", 8192, 1, 0, 4, 512), (True, "plain", 8195, 1, 0, 4, 513),
    (False, "plain", 4095, 0, 0, 1, 1024), (False, "plain", 4096, 1, 0, 2, 512), (False, "plain", 4099, 1, 0, 2, 513),
    (True, "swiglu", 4095, 0, 0, 1, 1024), (True, "swiglu", 4096, 1, 0, 2, 512), (True, "swiglu", 4099, 1, 0, 2, 513),
    (True, "residual", 4096, 0, 0, 1, 1024), (True, "inplace", 8195, 1, 0, 4, 513),
], ids=str)
def test_stream_wide_boundary(bf16, form, n_out, wide, loop, rpb, wgs):
    """Either side of the 16-loads-per-lane form at K = 2048, the upper one with a ragged last batch."""
    rt = gemv_case("stream wide", f"{DNAME[bf16]} K=2048 n={n_out} {form}", D.STREAM, rows=1, k=2048, n_out=n_out, bf16=bf16, form=form,
                   w_rows=8195 if bf16 and form != "swiglu" else 4099)
    assert (rt["wide"], rt["loop"], rt["rows_per_batch"], rt["workgroups"], rt["threads"]) == (wide, loop, rpb, wgs, 256)


@pytest.mark.parametrize("n_out,threads,wgs", [(2047, 256, 512), (2048, 512, 256), (2051, 512, 257)])
@pytest.mark.parametrize("form", ("residual", "rms"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_stream_512_threads(bf16, form, n_out, threads, wgs):
    """K = 8192: eight waves per workgroup from 2 048 batches on (the down projection's form)."""
    rt = gemv_case("stream 512", f"{DNAME[bf16]} K=8192 n={n_out} {form}", D.STREAM, rows=1, k=8192, n_out=n_out, bf16=bf16, form=form, w_rows=2051)
    assert (rt["threads"], rt["workgroups"], rt["loop"]) == (threads, wgs, 0)


@pytest.mark.parametrize("bf16,n_out,loop,wgs", [(True, 16384, 0, 1024), (True, 16400, 1, 512), (False, 8192, 0, 1024), (False, 8200, 1, 512)],
                         ids=lambda v: str(v))
def test_stream_looping_head(bf16, n_out, loop, wgs):
    """The vocabulary head: the last grid that covers its batches and the first that loops (ragged), RMSNorm and the normalised row."""
    rt = gemv_case("stream loop", f"{DNAME[bf16]} K=2048 n={n_out} rms+norm_out", D.STREAM, rows=1, k=2048, n_out=n_out, bf16=bf16, form="rms",
                   norm_out=True, w_rows=16400 if bf16 else 8200)
    assert (rt["loop"], rt["workgroups"], rt["wide"]) == (loop, wgs, 1)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_stream_looping_head_at_8192(bf16):
    """K = 8192 with more than 4 096 batches: the loop on eight-wave workgroups."""
    rt = gemv_case("stream loop", f"{DNAME[bf16]} K=8192 n=4100 plain", D.STREAM, rows=1, k=8192, n_out=4100, bf16=bf16, form="plain")
    assert (rt["loop"], rt["threads"], rt["workgroups"]) == (1, 512, 256)


@pytest.mark.parametrize("form", ("rms", "swiglu"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_stream_norm_out(k, bf16, form):
    gemv_case("stream", f"{DNAME[bf16]} K={k} {form} norm_out", D.STREAM, rows=1, k=k, n_out=9, bf16=bf16, form=form, norm_out=True)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_stream_swiglu_saturated_gate(k, bf16):
    """Gate sums of +-90: exp(90) overflows f32, silu(-90) * up must come out as (minus) zero and silu(90) as 90."""
    gemv_case("stream gate +-90", f"{DNAME[bf16]} K={k}", D.STREAM, rows=1, k=k, n_out=6, bf16=bf16, form="swiglu", gate=90.0)


@pytest.mark.parametrize("form", ("plain", "rms", "inplace"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_stream_probes_are_exact(k, bf16, form):
    """The largest entry at both ends of every 512-column piece (lane 0 / lane 63 of a piece) and of every thread's f32x4."""
    for j in edges(k, 512) + [3, 4, 1027, k // 2 + 257]:
        probe_case("stream probe", f"{DNAME[bf16]} K={k} {form}", D.STREAM, rows=1, k=k, n_out=9, bf16=bf16, form=form, cols=[j])


# ---- 2. split-K, one row, K not a streaming width ------------------------------------------------------------------------------------

SPLIT_K4 = (8, 264, 2040, 2056, 4088, 4104, 6144, 8184)      # four waves: 1, 1, 1, 2, 2, 4, 4, 4 chunks
SPLIT_K16 = (8200, 11008, 14336, 16384)                      # sixteen waves: 2 chunks
SPLIT_CH = {8: 1, 264: 1, 2040: 1, 2056: 2, 4088: 2, 4104: 4, 6144: 4, 8184: 4}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", SPLIT_K4 + SPLIT_K16)
def test_splitk_every_pair(k, bf16, form):
    i = (SPLIT_K4 + SPLIT_K16).index(k) + FORMS.index(form) + int(bf16)
    rt = gemv_case("splitk", f"{DNAME[bf16]} K={k} {form}", D.SPLITK, rows=1, k=k, n_out=(1, 2, 5)[i % 3], bf16=bf16, form=form, bias=i % 2 == 0,
                   scales=SMALL if i % 2 else None)
    assert (rt["ch"], rt["threads"]) == ((SPLIT_CH[k], 256) if k < 8192 else (2, 1024))


@pytest.mark.parametrize("n_out", (1, 2, 5))
@pytest.mark.parametrize("k", (2056, 4104, 14336))
def test_splitk_column_counts(k, n_out):
    for bf16 in DT:
        gemv_case("splitk", f"{DNAME[bf16]} K={k} n={n_out} rms", D.SPLITK, rows=1, k=k, n_out=n_out, bf16=bf16, form="rms")


@pytest.mark.parametrize("n_out", (1, 5))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (768, 2048))
def test_splitk_layernorm_gelu(k, bf16, n_out):
    """GPT-2's c_fc stage: LayerNorm + bias + GELU-tanh on one chunk of four waves."""
    rt = gemv_case("splitk ln+gelu", f"{DNAME[bf16]} K={k} n={n_out}", D.SPLITK, rows=1, k=k, n_out=n_out, bf16=bf16, form="ln+gelu")
    assert (rt["ch"], rt["threads"]) == (1, 256)


@pytest.mark.parametrize("form", ("plain", "rms", "residual"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (264, 2056, 4104, 8184, 8200, 16384))
def test_splitk_probes_are_exact(k, bf16, form):
    """Both ends of every chunk: 256 x 8 columns per chunk with four waves, 1 024 x 8 with sixteen, and of every wave's share."""
    step = 8192 if k >= 8192 else 2048
    for j in sorted(set(edges(k, step) + edges(k, 512))):
        probe_case("splitk probe", f"{DNAME[bf16]} K={k} {form}", D.SPLITK, rows=1, k=k, n_out=5, bf16=bf16, form=form, cols=[j])


# ---- 3. llm_gemv1_kernel, one row staged in LDS --------------------------------------------------------------------------------------

SEGS = ((1, 1), (3, 2), (9, 3), (6, 5))       # both boundaries in wave 0's and 1's pairs; inside workgroup 0's eight; across workgroups


@pytest.mark.parametrize("seg", (None,) + SEGS, ids=str)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (768, 1600))
def test_gemv1_layernorm_qkv(k, bf16, seg):
    n = seg[0] + 2 * seg[1] if seg else 9
    gemv_case("gemv1", f"{DNAME[bf16]} K={k} ln seg={seg}", D.ONE, rows=1, k=k, n_out=n, bf16=bf16, form="ln", seg=seg, row_off=3 if seg else 0,
              pads=(8, 2, 3, 0))


@pytest.mark.parametrize("on_device", (False, True), ids=("by-value", "on-device"))
@pytest.mark.parametrize("seg", SEGS, ids=str)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (72, 896, 16384))
def test_gemv1_rms_segments(k, bf16, seg, on_device):
    """RMSNorm + Q | K | V into the cache rows; K = 16 384 is the 64 KiB dynamic LDS limit."""
    row_off = (0, 2, 5)[(SEGS.index(seg) + int(on_device)) % 3]
    gemv_case("gemv1", f"{DNAME[bf16]} K={k} rms seg={seg} row_off={row_off} {'device' if on_device else 'value'}", D.ONE, rows=1, k=k,
              n_out=seg[0] + 2 * seg[1], bf16=bf16, form="rms", seg=seg, row_off=row_off, on_device=on_device, pads=(8, 1, 2, 0),
              scales=SMALL if on_device else None)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_gemv1_swiglu_with_segments(bf16):
    gemv_case("gemv1", f"{DNAME[bf16]} K=896 swiglu seg=(3, 2)", D.ONE, rows=1, k=896, n_out=7, bf16=bf16, form="swiglu", seg=(3, 2), row_off=1)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (72, 896, 16384))
def test_gemv1_probes_are_exact(k, bf16):
    """Both ends of every wave's 64 x 8-column trip and of the four trips a lane keeps in flight; the scatter at row_off 4."""
    for j in sorted(set(edges(k, 2048) + edges(k, 512))):
        probe_case("gemv1 probe", f"{DNAME[bf16]} K={k} rms seg=(9, 3)", D.ONE, rows=1, k=k, n_out=15, bf16=bf16, form="rms", cols=[j], seg=(9, 3),
                   row_off=4)


# ---- 4. llm_gemv_kernel, a wave per column, 1 - 8 rows -------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS + LN_FORMS)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("rows", (2, 3, 8))
def test_generic_every_pair(rows, bf16, form):
    """Every stride wider than its columns: ldx > k, ldy0 > n, ldr > n."""
    i = rows + (FORMS + LN_FORMS).index(form) + int(bf16)
    gemv_case("generic", f"{DNAME[bf16]} rows={rows} {form}", D.GENERIC, rows=rows, k=(72, 264, 520)[i % 3], n_out=(1, 3, 6)[i % 3], bf16=bf16,
              form=form, pads=(12, 3, 0, 5), scales=(1.0, 30.0, 0.03, 1.0, 5.0, 1.0, 0.2, 1.0))


@pytest.mark.parametrize("form", ("plain", "rms", "ln", "residual"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("rows", (2, 8))
def test_generic_segments(rows, bf16, form):
    """Segments with row_off > 0 and ldy12 > seg_kv, the offset by value and on the device."""
    on_device = (rows + int(bf16)) % 2 == 1
    gemv_case("generic", f"{DNAME[bf16]} rows={rows} {form} seg=(3, 2) {'device' if on_device else 'value'}", D.GENERIC, rows=rows, k=264, n_out=7,
              bf16=bf16, form=form, seg=(3, 2), row_off=2 if rows == 2 else 1, on_device=on_device, pads=(4, 1, 3, 2), cache_rows=10)


@pytest.mark.parametrize("form", ("plain", "rms", "swiglu", "ln", "ln+gelu"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_generic_one_long_row(bf16, form):
    """One row wider than every one-row kernel takes (K = 16 392), and GPT-2's c_fc stage past the split-K width."""
    k = 4096 if form == "ln+gelu" else 16392
    gemv_case("generic", f"{DNAME[bf16]} rows=1 K={k} {form}", D.GENERIC, rows=1, k=k, n_out=6, bf16=bf16, form=form)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_generic_segments_without_a_norm(bf16):
    gemv_case("generic", f"{DNAME[bf16]} rows=1 K=2048 plain seg=(9, 3)", D.GENERIC, rows=1, k=2048, n_out=15, bf16=bf16, form="plain", seg=(9, 3),
              row_off=3)


@pytest.mark.parametrize("form", ("plain", "rms", "inplace"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_generic_probes_are_exact(bf16, form):
    k = 520
    cols = edges(k, 512) + [255, 256]
    assert len(cols) == 8
    for three in (cols[0:3], cols[3:6], cols[5:8]):
        probe_case("generic probe", f"{DNAME[bf16]} K={k} rows=3 {form}", D.GENERIC, rows=3, k=k, n_out=6, bf16=bf16, form=form, cols=three)
    if form != "inplace":      # (segments take no in-place residual)
        probe_case("generic probe", f"{DNAME[bf16]} K={k} rows=8 {form} seg=(3, 2)", D.GENERIC, rows=8, k=k, n_out=7, bf16=bf16, form=form, cols=cols,
                   seg=(3, 2), row_off=1)


# ---- 5. launch_llm_gemv_lanes --------------------------------------------------------------------------------------------------------

LANE_K = (512, 768, 1024, 520, 1536, 2048, 2056, 3072, 8192, 14336)
LANE_FORM = {512: (2, 1), 768: (2, 1), 1024: (2, 1), 520: (2, 1), 1536: (4, 1), 2048: (4, 1), 2056: (2, 3), 3072: (2, 3), 8192: (4, 4), 14336: (4, 7)}
LANE_ROWS = (1, 2, 5, 8)
LANE_SCALES = (1.0, 40.0, 0.02, 3.0, 1.0, 0.1, 10.0, 1.0)      # a row's statistics applied to its neighbour fail


@pytest.mark.parametrize("form", FORMS + LN_FORMS)
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", LANE_K)
def test_lanes_every_pair(k, bf16, form):
    i = LANE_K.index(k) + (FORMS + LN_FORMS).index(form) + int(bf16)
    rt = gemv_case("lanes", f"{DNAME[bf16]} K={k} rows={LANE_ROWS[i % 4]} {form}", True, rows=LANE_ROWS[i % 4], k=k, n_out=(7, 1)[(i // 4) % 2],
                   bf16=bf16, form=form, lanes=True, pads=(4, 2, 0, 3), scales=LANE_SCALES)
    assert (rt["ch"], rt["ns"], rt["wide"], rt["cpw"]) == LANE_FORM[k] + (0, 1)


@pytest.mark.parametrize("rows", LANE_ROWS)
@pytest.mark.parametrize("k", (520, 1536, 2056, 3072))
def test_lanes_every_row_count(k, rows):
    for bf16, form in ((False, "rms"), (True, "swiglu")):
        gemv_case("lanes", f"{DNAME[bf16]} K={k} rows={rows} {form}", True, rows=rows, k=k, n_out=7, bf16=bf16, form=form, lanes=True, scales=LANE_SCALES)


@pytest.mark.parametrize("form", ("plain", "rms", "ln"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("rows", (2, 5))
def test_lanes_fallback_below_512(rows, bf16, form):
    """K = 504: the lanes kernel does not take it, launch_llm_gemv does and `streamed` says so."""
    rt = gemv_case("lanes fallback", f"{DNAME[bf16]} K=504 rows={rows} {form}", False, rows=rows, k=504, n_out=7, bf16=bf16, form=form, lanes=True)
    assert rt["streamed"] == 0 and rt["fallback"]["kernel"] == D.GENERIC


@pytest.mark.parametrize("bf16,k,n_out,form,wide,cpw,wgs", [
    (True, 2048, 2052, "rms", 0, 1, 512), (False, 1024, 2052, "plain", 0, 1, 512),       # one slice, 513 batches on 512 workgroups
    (True, 2048, 8176, "plain", 0, 1, 512), (True, 2048, 8177, "plain", 1, 4, 512),
    (False, 2048, 4088, "rms", 0, 1, 512), (False, 2048, 4089, "rms", 1, 2, 512),
    (True, 2048, 4089, "swiglu", 1, 2, 512), (True, 1024, 8177, "residual", 1, 4, 512),
    (True, 3072, 8177, "rms", 1, 4, 512),                                                # three slices, four columns per wave
], ids=str)
def test_lanes_loop_and_wide_boundary(bf16, k, n_out, form, wide, cpw, wgs):
    rt = gemv_case("lanes wide", f"{DNAME[bf16]} K={k} n={n_out} rows=3 {form}", True, rows=3, k=k, n_out=n_out, bf16=bf16, form=form, lanes=True,
                   scales=LANE_SCALES, w_rows=8177 if bf16 else 4089)
    assert (rt["wide"], rt["cpw"], rt["workgroups"]) == (wide, cpw, wgs)


@pytest.mark.parametrize("form", ("rms", "ln", "plain"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k,rows", ((768, 2), (2056, 5), (8192, 8)))
def test_lanes_segments_with_the_offset_on_the_device(k, rows, bf16, form):
    gemv_case("lanes", f"{DNAME[bf16]} K={k} rows={rows} {form} seg=(3, 2) device", True, rows=rows, k=k, n_out=7, bf16=bf16, form=form, lanes=True,
              seg=(3, 2), row_off=2, on_device=True, pads=(4, 1, 3, 0), cache_rows=12, scales=LANE_SCALES)
    gemv_case("lanes", f"{DNAME[bf16]} K={k} rows={rows} {form} seg=(9, 3) value", True, rows=rows, k=k, n_out=15, bf16=bf16, form=form, lanes=True,
              seg=(9, 3), row_off=4, pads=(4, 0, 1, 0), cache_rows=12, scales=LANE_SCALES)


def lane_probe_cols(k, ch):
    """Both ends of every slice, of every 512-column piece and of the tail pieces past the end of K."""
    return sorted(set(edges(k, ch * 512) + edges(k, 512)))


@pytest.mark.parametrize("form", ("plain", "rms", "inplace"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (520, 1536, 2056, 3072, 8192))
def test_lanes_probes_are_exact(k, bf16, form):
    """Eight rows, each with its largest entry at another edge: a row of weights read at a wrapped or stale column, an accumulator
    kept from the batch or slice before, or a row's slice taken for another row gives another integer."""
    cols = lane_probe_cols(k, LANE_FORM[k][0])
    cols += [c + 1 for c in cols if c + 1 < k][:(-len(cols)) % 8]
    for c in range(0, len(cols), 8):
        probe_case("lanes probe", f"{DNAME[bf16]} K={k} rows=8 {form}", True, rows=8, k=k, n_out=21, bf16=bf16, form=form, cols=cols[c:c + 8], lanes=True,
                   salt=c)
    if LANE_FORM[k][1] == 1:   # one slice: 513 batches on 512 workgroups, the first workgroup takes two
        probe_case("lanes probe", f"{DNAME[bf16]} K={k} rows=5 {form} n=2052", True, rows=5, k=k, n_out=2052, bf16=bf16, form=form, cols=cols[-5:],
                   lanes=True)


# ---- 6. launch_llm_qkv_rope ----------------------------------------------------------------------------------------------------------

GEOMS = ((3, 1, 6), (4, 2, 64), (5, 1, 32), (2, 2, 80), (14, 2, 128))
POSITIONS, CACHE_ROWS = 7, 9


def tables(d, seed=0):
    ang = np.random.default_rng([d, seed]).uniform(-math.pi, math.pi, (POSITIONS, d // 2))
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


def qkv_case(group, case, kernel, *, k, geom, bf16, bias, pos, on_device=False, embed=None, vocab=5, x_raw=True, seed=0):
    ops = _ops()
    heads, kv, d = geom
    n = (heads + 2 * kv) * d
    rng = np.random.default_rng([seed, k, heads, kv, d, int(bf16)])
    w = mat(n, k, bf16, seed=2)
    gamma = gamma_of(rng, k)
    b = (0.5 * rng.standard_normal(n)).astype(F32) if bias else None
    cos_t, sin_t = tables(d)
    table = x = None
    if embed is None:
        x = (rng.standard_normal(k) * (1.0 if bias else SMALL[0])).astype(F32)
        xin = x
    else:
        t = rng.standard_normal((vocab, k)).astype(F32)
        table = ops.to_bf16(t) if bf16 else t
        xin = D.embed_row(table, embed, bf16)
    q0, kc0, vc0 = nans(heads * d), nans(CACHE_ROWS, kv * d), nans(CACHE_ROWS, kv * d)
    xr0 = nans(k) if embed is not None and x_raw else None
    kw = dict(x=x, embed_id=embed, table=table, eps=EPS, bf16=bf16, bias=b, offset_on_device=on_device, x_raw_out=xr0)
    q, kc, vc, xr, rt = ops.llm_qkv_rope(w, gamma, heads, kv, d, cos_t, sin_t, pos, q0, kc0, vc0, **kw)
    q2, kc2, vc2, xr2, rt2 = ops.llm_qkv_rope(w, gamma, heads, kv, d, cos_t, sin_t, pos, q0, kc0, vc0, **kw)
    assert rt == rt2 and all(np.array_equal(bits(a), bits(c)) for a, c in ((q, q2), (kc, kc2), (vc, vc2))), f"{group} {case}: two runs differ"
    assert rt == D.qkv_route(k, heads, kv, d, embed=embed is not None) and rt["kernel"] == kernel, (case, rt)
    rq, rk, rv = D.qkv_rope64(xin, gamma, EPS, w, b, heads, kv, d, cos_t, sin_t, pos, bf16=bf16)
    check(group, case + " Q", q[None, :], rq[None, :])
    check(group, case + " K", kc, rk[None, :], pos)         # (every other cache row must still hold the pattern)
    check(group, case + " V", vc, rv[None, :], pos)
    if xr0 is not None:
        assert np.array_equal(bits(xr), bits(xin)), f"{group} {case}: x_raw_out is not the embedding row"
        assert np.array_equal(bits(xr), bits(xr2))
    return rt, (q, kc, vc)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k,ch", ((8, 1), (264, 1), (2040, 1), (2056, 2), (4104, 4), (8184, 4)))
def test_qkv_pair_kernel(k, ch, bf16):
    i = (8, 264, 2040, 2056, 4104, 8184).index(k) + int(bf16)
    rt, _ = qkv_case("qkv pair", f"{DNAME[bf16]} K={k} {GEOMS[i % 4]}", D.PAIR, k=k, geom=GEOMS[i % 4], bf16=bf16, bias=i % 2 == 0, pos=(0, 1, 6)[i % 3],
                     on_device=i % 2 == 1)
    assert rt["ch"] == ch


@pytest.mark.parametrize("bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("on_device", (False, True), ids=("by-value", "on-device"))
@pytest.mark.parametrize("pos", (0, 1, POSITIONS - 1))
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_qkv_geometry(geom, pos, on_device, bias):
    """Task counts that are no multiple of 4, a head_dim that is no power of two, every position form: the per-pair kernel at
    K = 264 and the streaming kernel at K = 2048, f32 and bf16 in turn."""
    i = GEOMS.index(geom) + pos + int(on_device) + int(bias)
    qkv_case("qkv pair", f"{DNAME[i % 2 == 0]} K=264 {geom} pos={pos} dev={int(on_device)} bias={int(bias)}", D.PAIR, k=264, geom=geom, bf16=i % 2 == 0,
             bias=bias, pos=pos, on_device=on_device)
    qkv_case("qkv stream", f"{DNAME[i % 2 == 1]} K=2048 {geom} pos={pos} dev={int(on_device)} bias={int(bias)}", D.QKV_STREAM, k=2048, geom=geom,
             bf16=i % 2 == 1, bias=bias, pos=pos, on_device=on_device)


@pytest.mark.parametrize("embed", (None, 0, 4, 5), ids=("x", "id0", "id-last", "id-vocab"))
@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", STREAM_K)
def test_qkv_stream_kernel_and_the_gather(k, bf16, embed):
    """With x, or gathering row 0, vocab - 1 or vocab of the table: the last leaves zeros in x_raw_out and a Q / K / V of bias alone.
    (K = 2048 / 4096 with f32 weights: the launcher's rule sends them to the streaming kernel too, and the route says so.)"""
    i = STREAM_K.index(k) + int(bf16) + (embed or 0)
    geom = GEOMS[(0, 2, 3)[i % 3]]
    kind = D.QKV_STREAM if embed is None else D.QKV_STREAM_EMBED
    rt, (q, kc, vc) = qkv_case("qkv stream", f"{DNAME[bf16]} K={k} {geom} embed={embed}", kind, k=k, geom=geom, bf16=bf16, bias=True, pos=(1, 6, 0)[i % 3],
                               on_device=i % 2 == 0, embed=embed)
    assert rt["ch"] == k // 512 and rt["workgroups"] == ((geom[0] + 2 * geom[1]) * geom[2] // 2 + 3) // 4


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
def test_qkv_gather_without_x_raw_out_and_without_bias(bf16):
    qkv_case("qkv stream", f"{DNAME[bf16]} K=2048 (5, 1, 32) embed=2 plain", D.QKV_STREAM_EMBED, k=2048, geom=(5, 1, 32), bf16=bf16, bias=False, pos=3,
             embed=2, x_raw=False)


@pytest.mark.parametrize("bf16", DT, ids=DNAME.get)
@pytest.mark.parametrize("k", (264, 2056, 8184, 2048, 8192))
def test_qkv_probes_are_exact(k, bf16):
    """Integer weights and bias, probe rows (RMSNorm divides by exactly 1), table rows (cos, sin) = (1, 0), (0, 1), (-1, 0): every
    Q / K / V element is an integer sum, moved or negated by the rotation and nothing else."""
    ops = _ops()
    heads, kv, d = 3, 1, 6
    n, half = (heads + 2 * kv) * d, d // 2
    w, wi = int_mat(n, k, bf16, salt=3)
    bi = (np.arange(n, dtype=np.int64) * 5) % 9 - 4
    cs = np.array([[1, 0], [0, 1], [-1, 0]], np.int64)
    cos_t, sin_t = (np.repeat(cs[:, i:i + 1], half, axis=1).astype(F32) for i in (0, 1))
    kind = D.PAIR if k not in STREAM_K else D.QKV_STREAM
    for j in sorted(set(edges(k, 2048) + edges(k, 512))):
        xi = probe_row(k, j)
        y = wi @ xi + bi
        pos = j % 3
        c, s = cs[pos]

        def rot(v, nh):
            h = v.reshape(nh, d)
            return np.concatenate([h[:, :half] * c - h[:, half:] * s, h[:, :half] * s + h[:, half:] * c], axis=1).reshape(-1)

        q, kc, vc, _, rt = ops.llm_qkv_rope(w, np.ones(k, F32), heads, kv, d, cos_t, sin_t, pos, nans(heads * d), nans(4, kv * d), nans(4, kv * d),
                                            x=xi.astype(F32), eps=0.0, bf16=bf16, bias=bi.astype(F32))
        assert rt["kernel"] == kind
        for name, got, want in (("Q", q, rot(y[:heads * d], heads)), ("K", kc[pos], rot(y[heads * d:(heads + kv) * d], kv)),
                                ("V", vc[pos], y[(heads + kv) * d:])):
            assert np.array_equal(got, want.astype(F32)), f"qkv probe {DNAME[bf16]} K={k} column {j} pos {pos}: {name} {got} != {want}"
        others = [r for r in range(4) if r != pos]
        untouched("qkv probe", f"K={k} column {j}", kc[others])
        untouched("qkv probe", f"K={k} column {j}", vc[others])


# ---- the refusals reach the caller as exceptions, with the arrays as they were ------------------------------------------------------

def test_refusals_leave_the_outputs_alone():
    from kjarni_amd._ffi import KjarniException
    ops = _ops()
    x, w, y = np.ones((2, 16), F32), np.ones((6, 16), F32), nans(2, 6)
    for kw in (dict(gamma=np.ones(16, F32), r=np.ones((2, 6), F32)), dict(swiglu=True, gamma=np.ones(16, F32)), dict(gelu_tanh=True),
               dict(norm_out=nans(16), gamma=np.ones(16, F32)), dict(seg_q=2, seg_kv=1)):
        with pytest.raises(KjarniException):
            ops.llm_gemv(x, w, 2, [y], **kw)
    t = np.ones((4, 2), F32)
    with pytest.raises(KjarniException):
        ops.llm_qkv_rope(np.ones((16, 16), F32), np.ones(16, F32), 2, 1, 4, t, t, 4, nans(8), nans(4, 4), nans(4, 4), x=np.ones(16, F32))
    untouched("refusals", "y", y)


def test_report_the_largest_errors():
    """Not a check: prints the largest error of every group as a fraction of its bar (also in the terminal summary)."""
    for group, (ratio, err, bar, case) in sorted(WORST.items()):
        print(f"[dense_proj] {group}: largest err {err:.3e} (bar {bar:.3e}, {ratio:.2f} of it) at {case}")
