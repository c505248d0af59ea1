"""The FP8 prompt GEMM on the bf16 matrix cores (prefill_gemm_fp8w_kernel through kjarni_hip_op_prefill_gemm_fp8) and the switch
that routes FP8 checkpoints onto it (set_fp8_matrix_cores): the prompt route and the wide lanes.

The kernel alone.  Every call runs twice and must give the same bits.  Everything the kernel may over-read but must not use is NaN
beforehand (A's rows behind m and its padding columns, the split scratch), the padding columns of Y are NaN and must stay NaN, the
hook keeps a guard band behind every device buffer.  Bar: the project's for FP8 projections, 1e-5 * max(1, max |ref|) against
float64 of decode(code) * scale (tests/fp8_gemm_ref64.py); the exact cases are compared bit for bit.

Whole models (tests/wide_fp8_cases.py) run with the switch on against llm_ref64 / qwen3_ref64 at llm_ref64.TOL; token ids are
compared at steps whose two best reference logits are more than 100 bars apart, which every compared step is asserted to be."""
import numpy as np
import pytest

from kjarni_amd import ops
from tests import fp8_fixture as F
from tests import fp8_gemm_ref64 as R
from tests import prefill_ref64 as P

pytestmark = pytest.mark.gpu

NAN = np.float32(np.nan)
KINDS = F.KINDS


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _padded(rows, m, k, pad_rows=3, pad_cols=0):
    """rows [m, k] inside a NaN array [m + pad_rows, k + pad_cols]."""
    a = np.full((m + pad_rows, k + pad_cols), NAN, np.float32)
    a[:m, :k] = rows
    return a


def _call(a, codes, scale, kind, m, n, pad_y=0, y0=None, want_written=None, **kw):
    """The hook twice on the same arguments: the same bits.  Returns (y, gate, ksplit_used, scratch words written or None)."""
    n_, k = codes.shape
    assert n_ == n
    s2 = np.asarray(scale, np.float32).reshape(F.scale_shape(kind, n, k))
    y = np.full((m, n + pad_y), NAN, np.float32) if y0 is None else y0
    split = kw.pop("split", True)
    want_written = split if want_written is None else want_written
    outs = [ops.prefill_gemm_fp8(a, codes, s2, m, y, split=split, want_scratch_written=want_written, **kw) for _ in range(2)]
    for x, z in zip(outs[0][:2], outs[1][:2]):
        assert (x is None and z is None) or np.array_equal(_bits(x), _bits(z)), "two runs of the same call differ"
    assert outs[0][2:] == outs[1][2:]
    o = outs[0]
    return o[0], o[1], o[2], (o[3] if want_written else None)


def _check(name, got, ref):
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), f"{name}: NaN / inf in the result: an over-read row, padding or the scratch's poison was used"
    err, bar = float(np.abs(got.astype(np.float64) - ref).max()), R.bar(ref)
    print(f"{name}: max |kernel - float64| = {err:.3e} (bar {bar:.3e})")
    assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    return err


def _random_codes(rng, n, k):
    return F.FINITE_CODES[rng.integers(0, len(F.FINITE_CODES), (n, k))]


# ---- exact decode -------------------------------------------------------------------------------------------------------------------

def test_every_code_is_decoded_exactly():
    """All 254 finite codes spread through W [64, 256]; A = the 256 one-hot rows: y[i, j] is W[j, i]'s value, bit for bit -- with
    scale 1, and with scale 0.75 as the f32 product decode * 0.75."""
    n, k = 64, 256
    codes = np.resize(F.FINITE_CODES, n * k).reshape(n, k).copy()
    codes = codes[:, np.random.default_rng(0).permutation(k)]          # (every code at several columns, chunks and lanes)
    assert set(codes.ravel().tolist()) == set(F.FINITE_CODES.tolist())
    a = _padded(np.eye(k, dtype=np.float32), k, k)
    for scale in (1.0, 0.75):
        want = (F.TABLE[codes].T * np.float32(scale)).astype(np.float32)
        for split in (True, False):
            y, _, used, _ = _call(a, codes, np.float32([scale]), "tensor", k, n, split=split)
            assert used == (2 if split else 1)
            bad = np.nonzero(_bits(y) != _bits(want))
            # (-0 codes: 0 * x sums give +0 in the accumulator; the value is compared, the sign of zero is not a weight)
            assert np.array_equal(y, want) and (np.signbit(y) == np.signbit(want))[want != 0].all(), (scale, split, bad[0][:4], bad[1][:4])


# ---- against float64 ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_gemm_fp8_against_float64(kind):
    """k below one K slice, with a slice boundary inside a block, at eight slices, four blocks per slice; m of one row, partial
    tiles, one tile exactly, one row more, three tiles; n below a tile, one tile, and 200: the last 64-column tile partial and the
    second row of blocks 72 rows tall."""
    rng = np.random.default_rng(10 + KINDS.index(kind))
    worst = 0.0
    for k in (128, 384, 2048, 8192):
        for n in (8, 64, 200):
            codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
            w64 = R.weights64(codes, scale, kind)
            for m in (1, 9, 33, 64, 65, 130):
                x = rng.standard_normal((m, k)).astype(np.float32)
                y, _, used, written = _call(_padded(x, m, k, pad_cols=4), codes, scale, kind, m, n, pad_y=4)
                assert used == P.ksplit_rule(m, n, k) and written == (used * m * n if used > 1 else 0)
                assert np.isnan(y[:, n:]).all(), "the padding columns of Y were written"
                err = _check(f"{kind} k={k} n={n} m={m}", y[:, :n], x.astype(np.float64) @ w64.T)
                worst = max(worst, err / R.bar(x.astype(np.float64) @ w64.T))
    print(f"{kind}: worst error / bar = {worst:.3f}")


def _far_block_scales(rng, n, k):
    """Block scales whose neighbours in k and in n differ by a factor of about 2^6 (2^5.4 .. 2^6.6), up or down."""
    rows, cols = F.scale_shape("block", n, k)
    e = np.array([[3 if (i + j) % 2 == 0 else -3 for j in range(cols)] for i in range(rows)], np.float64)
    return (2.0 ** e * rng.uniform(0.8, 1.25, (rows, cols)) * 0.01).astype(np.float32)


@pytest.mark.parametrize("k,split", [(384, True), (384, False), (512, True), (1024, True), (256, False)])
def test_block_scales_far_apart(k, split):
    """One wrong block index is thousands of bars off.  k = 384 split: two slices of 192, the boundary inside block 1."""
    rng = np.random.default_rng(k + int(split))
    n, m = 200, 65
    scale = _far_block_scales(rng, n, k)
    assert (np.abs(np.log2(scale[:, 1:] / scale[:, :-1])) > 5).all() and (np.abs(np.log2(scale[1:] / scale[:-1])) > 5).all()
    assert scale.shape == (2, k // 128)
    codes = _random_codes(rng, n, k)
    x = rng.standard_normal((m, k)).astype(np.float32)
    y, _, used, _ = _call(_padded(x, m, k), codes, scale, "block", m, n, split=split)
    assert used == (P.ksplit_rule(m, n, k) if split else 1) and (used > 1) == split
    _check(f"far block scales k={k} split={split}", y, R.gemm64(x, codes, scale, "block"))


# ---- K splits -----------------------------------------------------------------------------------------------------------------------

SPLIT_TABLE = [(63, 60, 96, 1), (64, 64, 192, 1), (65, 68, 256, 2), (33, 64, 384, 2), (33, 64, 512, 4), (70, 196, 768, 4), (64, 128, 1024, 8),
               (1, 4, 1024, 8), (24, 37, 1024, 1), (65, 4160, 1024, 4)]
# (block scales need k % 128 == 0; the launcher refuses the others: tests/test_fp8_gemm_host.py)
SPLIT_CASES = [(kind,) + c for kind in KINDS for c in SPLIT_TABLE if kind != "block" or c[2] % 128 == 0]


@pytest.mark.parametrize("kind,m,n,k,want", SPLIT_CASES, ids=str)
def test_k_splits(kind, m, n, k, want):
    """Splits of 1, 2, 4 and 8 (and n % 4, which takes none) against the rule restated in tests/prefill_ref64.py."""
    rng = np.random.default_rng(m + n + k)
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    x = rng.standard_normal((m, k)).astype(np.float32)
    y, _, used, written = _call(_padded(x, m, k), codes, scale, kind, m, n)
    assert used == want == P.ksplit_rule(m, n, k)
    assert written == (used * m * n if used > 1 else 0), "partial tiles: every element once; unsplit: the scratch untouched"
    _check(f"{kind} {m}x{n}x{k} ksplit {used}", y, R.gemm64(x, codes, scale, kind))
    y1, _, one, _ = _call(_padded(x, m, k), codes, scale, kind, m, n, split=False)
    assert one == 1
    _check(f"{kind} {m}x{n}x{k} unsplit", y1, R.gemm64(x, codes, scale, kind))


# ---- epilogues ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["channel", "block"])
@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
@pytest.mark.parametrize("epilogue", ["bias", "residual", "inplace", "bias+inplace", "gate"])
def test_epilogues(epilogue, split, kind):
    """The scale comes before the bias (a bias of 50 against products of ~1: scaling it would show), the residual apart (ldr > n) and
    in place, and the SwiGLU fold with gate values at +-90 among the others: in the reduce kernel (split) and behind the tile kernel."""
    m, n, k = 70, 196, 768
    rng = np.random.default_rng(len(epilogue) * 4 + int(split) * 2 + KINDS.index(kind))
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    x = rng.standard_normal((m, k)).astype(np.float32)
    a = _padded(x, m, k)
    bias = (50.0 * rng.standard_normal(n)).astype(np.float32) if "bias" in epilogue else None
    y0 = np.full((m, n + 4), NAN, np.float32)
    r = r_ref = gate = None
    if epilogue == "residual":
        r = np.full((m, n + 8), NAN, np.float32)
        r[:, :n] = rng.standard_normal((m, n)).astype(np.float32)
        r_ref = r[:, :n]
    elif "inplace" in epilogue:
        y0[:, :n] = rng.standard_normal((m, n)).astype(np.float32)
        r_ref = y0[:, :n].copy()
    elif epilogue == "gate":
        y0 = np.full((m, n), NAN, np.float32)
        gate = rng.standard_normal((m, n)).astype(np.float32)
        gate[::7, ::5] = 90.0
        gate[3::7, 2::5] = -90.0
    y, g, used, _ = _call(a, codes, scale, kind, m, n, y0=y0, bias=bias, r=r, r_is_y="inplace" in epilogue, gate=gate, split=split)
    assert (used > 1) == split
    name = f"{kind} {epilogue} {'split' if split else 'unsplit'}"
    if epilogue == "gate":
        ref_y, ref_g = R.gemm64(x, codes, scale, kind, gate=gate)
        _check(name + " fold", g, ref_g)
        if used > 1:
            assert np.isnan(y).all(), "a split SwiGLU launch leaves Y alone"
        else:
            _check(name + " product", y, ref_y)
        return
    assert np.isnan(y[:, n:]).all()
    _check(name, y[:, :n], R.gemm64(x, codes, scale, kind, bias, r_ref))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
def test_a_middle_segment_of_wider_rows(split, kind):
    """ldy = n + 96 with the output 48 columns into the rows -- the wide step's Q | K | V layout: everything outside stays NaN."""
    m, n, k, off = 33, 64, 256, 48
    rng = np.random.default_rng(7 + KINDS.index(kind))
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    x = rng.standard_normal((m, k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    ld = n + 96
    whole = np.full((m + 1, ld), NAN, np.float32)
    view = whole.ravel()[off:off + m * ld].reshape(m, ld)                # row r of the view starts at column 48 of row r
    y, _, used, _ = _call(_padded(x, m, k), codes, scale, kind, m, n, y0=view, bias=bias, split=split)
    assert used == (2 if split else 1)
    got = np.full((m + 1, ld), NAN, np.float32)
    got.ravel()[off:off + m * ld] = y.ravel()
    _check(f"{kind} middle segment", got[:m, off:off + n], R.gemm64(x, codes, scale, kind, bias))
    outside = np.ones((m + 1, ld), bool)
    outside[:m, off:off + n] = False
    assert np.isnan(got[outside]).all(), "columns outside the segment were written"


# ---- integer probes -----------------------------------------------------------------------------------------------------------------

def _int_codes(rng, n, k):
    """Codes of the integers -8 .. 8 (exact in e4m3)."""
    vals = rng.integers(-8, 9, (n, k)).astype(np.float64)
    codes = F.encode(vals)
    assert np.array_equal(F.TABLE[codes].astype(np.float64), vals)
    return codes


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,split", [(384, True), (384, False), (1024, True), (256, True)])
def test_integer_probes_at_slice_and_block_edges(k, split, kind):
    """Integer activations that are non-zero only at the first and last k of every slice and every 128-block, integer codes,
    power-of-two scales: every sum is exact in f32, so the result equals the float64 one exactly -- a k that is skipped, read twice
    or scaled by a neighbour's block shows as a whole number."""
    m, n = 65, 136
    rng = np.random.default_rng(k)
    used_want = P.ksplit_rule(m, n, k) if split else 1
    edges = set()
    for step in (k // used_want, 128, 32):
        for s in range(0, k, step):
            edges |= {s, s + step - 1}
    cols = np.array(sorted(edges))
    x = np.zeros((m, k), np.float32)
    x[:, cols] = rng.integers(-4, 5, (m, len(cols))).astype(np.float32)
    x[:, cols[0]] = 1.0
    codes = _int_codes(rng, n, k)
    shape = F.scale_shape(kind, n, k)
    scale = (2.0 ** rng.integers(-3, 4, shape)).astype(np.float32)
    y, _, used, _ = _call(_padded(x, m, k), codes, scale, kind, m, n, split=split)
    assert used == used_want
    want = R.gemm64(x, codes, scale, kind)
    assert np.array_equal(y.astype(np.float64), want), np.nonzero(y != want)


def test_all_three_planes_of_the_activations_count():
    """A = diag(v) with full 24-bit significands in [1, 2), every finite code in W, scale 1: y[i, j] = v[i] * w[j, i] through the three
    plane products p3 w + p2 w + p1 w, each exact (8 x 4 bits), added in f32 with two roundings of at most 2^-24 of the sum --
    bound 2^-22 |ref| per element.  Without the third plane the result is off by |p3 w|, up to 2^-17 |ref|; without the second by
    2^-9: the 1e-5 bar of the random cases sees neither."""
    n, k = 64, 256
    rng = np.random.default_rng(12)
    codes = np.resize(F.FINITE_CODES, n * k).reshape(n, k)[:, rng.permutation(k)].copy()
    v = (1.0 + rng.integers(0, 1 << 23, k).astype(np.float64) / (1 << 23)).astype(np.float32)
    u = v.view(np.uint32)
    assert ((u & 0xFF) != 0).sum() > 200, "precondition: the low significand bits (the third plane) are in use"
    y, _, used, _ = _call(_padded(np.diag(v), k, k), codes, np.float32([1.0]), "tensor", k, n)
    assert used == 2
    ref = v.astype(np.float64)[:, None] * F.TABLE[codes].T.astype(np.float64)
    err = np.abs(y.astype(np.float64) - ref)
    assert (err <= 2.0 ** -22 * np.abs(ref)).all(), float((err / np.maximum(np.abs(ref), 1e-300)).max())


# ---- row independence, the parent's route ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_a_row_is_the_same_at_9_and_64_rows(kind):
    """One M tile and the same K split either way: a row's bits do not depend on how many rows ride along."""
    n, k = 200, 512
    rng = np.random.default_rng(3)
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    x = rng.standard_normal((64, k)).astype(np.float32)
    y9, _, u9, _ = _call(_padded(x[:9], 9, k), codes, scale, kind, 9, n)
    y64, _, u64, _ = _call(_padded(x, 64, k), codes, scale, kind, 64, n)
    assert u9 == u64 == 4
    assert np.array_equal(_bits(y9), _bits(y64[:9]))


@pytest.mark.parametrize("kind", KINDS)
def test_against_the_dequantizing_route(kind):
    """kjarni_hip_op_linear_fp8 at m >= 24 is launch_fp8_dequant + the f32 GEMM, the route the switch replaces: each is within a bar
    of float64, so they agree within two."""
    import ctypes as C

    import kjarni_amd
    n, k = 200, 2048
    rng = np.random.default_rng(4)
    codes, scale = F.quantize(rng.standard_normal((n, k)).astype(np.float32) * 0.05, kind, rng)
    for m in (24, 65):
        x = rng.standard_normal((m, k)).astype(np.float32)
        y, _, _, _ = _call(_padded(x, m, k), codes, scale, kind, m, n)
        old = np.empty((m, n), np.float32)
        rows, cols = F.scale_shape(kind, n, k)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        s = np.ascontiguousarray(scale, np.float32)
        rc = kjarni_amd.lib().kjarni_hip_op_linear_fp8(0, fp(x), m, codes.ctypes.data_as(C.c_void_p), fp(s), rows, cols, n, k, fp(old))
        assert rc == 0, kjarni_amd._ffi.last_error()
        ref = R.gemm64(x, codes, scale, kind)
        _check(f"{kind} m={m} new", y, ref)
        assert float(np.abs(y.astype(np.float64) - old).max()) <= 2 * R.bar(ref)


# ---- whole models with the switch on ------------------------------------------------------------------------------------------------
# tests/wide_fp8_cases.py: llama per tensor, llama per channel, qwen2 per channel with biases, qwen3 block, mistral block.

import os  # noqa: E402
import shutil  # noqa: E402

from tests import llm_ref64 as R64  # noqa: E402
from tests import wide_fp8_cases as WF  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_NAMES = list(WF.MODELS)
REFUSAL = "checkpoint: the prompt GEMM would dequantize every matrix in every step (8 lanes or fewer run it)"


class _Ref:
    """The float64 reference behind test_gpu_wide_lanes._run_wide_steps' interface."""

    def __init__(self, ref, cfg):
        self.ref, self.vocab, self.first_id = ref, cfg["vocab_size"], 4

    def new(self):
        return self.ref.new_cache()

    def forward(self, ids, state):
        h = self.ref.forward(list(ids), state)[-1:]
        return self.ref.rms_norm(h, self.ref.t["model.norm.weight"])[0], WF.logits64(self.ref, h)[0]

    def cache(self, state):
        return state


class _Fp8Case:
    def __init__(self, tmp, name):
        import kjarni_amd
        geo, kind, seed = WF.MODELS[name]
        self.name, self.dir = name, str(tmp / "fp8")
        self.cfg, self.hf = F.fp8_model(self.dir, dict(geo), kind, seed=seed)
        self.ref = WF.reference(name, self.hf, self.cfg)
        self.dec = kjarni_amd.HipDecoder(self.dir)
        assert self.dec.weight_bytes_by_type().get("F8_E4M3", 0) > 0
        assert not self.dec.fp8_matrix_cores(), "the switch is off by default"
        self.dec.set_fp8_matrix_cores(True)
        assert self.dec.fp8_matrix_cores()
        self.ps, self.news = WF.case(name)
        self._exp = None

    @property
    def exp(self):
        """The float64 ids of the 72 prompts, computed once; every step's margin is asserted here, none is left out."""
        if self._exp is None:
            self._exp = [WF.clear_greedy(self.ref, self.cfg, p, m, f"{self.name} prompt {i}") for i, (p, m) in enumerate(zip(self.ps, self.news))]
        return self._exp


@pytest.fixture(scope="module")
def fp8_cases(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Fp8Case(tmp_path_factory.mktemp(name.replace("-", "_")), name)
        made[name].dec.set_fp8_matrix_cores(True)
        return made[name]
    return get


def _within64(got, ref, what):
    ref = np.asarray(ref, np.float64)
    err, bar = float(np.abs(np.asarray(got, np.float64) - ref).max()), R64.TOL * max(1.0, float(np.abs(ref).max()))
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("n", [9, 33, 64])
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_wide_steps_against_float64(fp8_cases, name, n):
    """Every live lane's hidden row, logits row and K / V rows at every step, ragged positions, prompts prefilled by 8-row passes
    and by the FP8 prompt GEMM, a lane that fills its cache and frozen lanes found unrewritten bit for bit."""
    from tests.test_gpu_wide_lanes import _run_wide_steps
    c = fp8_cases(name)
    freeze = (2, 7, n - 1)
    frozen = _run_wide_steps(c.dec, _Ref(c.ref, c.cfg), n, seed=100 + n, freeze=freeze)
    assert set(freeze) | {5} <= set(frozen) and frozen[5][0] == 64


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_generate_wide_equals_generate_and_the_reference(fp8_cases, name):
    c = fp8_cases(name)
    assert len(c.ps) == 72 and all(4 <= m <= 10 for m in c.news)
    single = [c.dec.generate(p, m) for p, m in zip(c.ps, c.news)]
    assert single == c.exp
    for lanes in (9, 64):
        for again in range(2):                                           # the second call replays the captured step graphs
            assert c.dec.generate_wide(c.ps, c.news, lanes=lanes, lane_context=WF.LANE_CONTEXT) == c.exp, (lanes, again)
    assert c.dec.generate_wide(c.ps[:12], c.news[:12], lanes=8, lane_context=WF.LANE_CONTEXT) == c.exp[:12]      # the 8-lane route


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_prompt_route_against_float64_and_the_switch_off(fp8_cases, name):
    c = fp8_cases(name)
    dec, cfg = c.dec, c.cfg
    rng = np.random.default_rng(11)
    for n in (24, 64, 130):                                              # one partial M tile, one tile exactly, three tiles
        ids = rng.integers(4, cfg["vocab_size"], n).tolist()
        cache64 = c.ref.new_cache()
        want = WF.logits64(c.ref, c.ref.forward(ids, cache64)[-1:])[0]
        out = {}
        for on in (True, False):
            dec.set_fp8_matrix_cores(on)
            dec.reset()
            _, logits = dec.forward(ids)
            rows = [dec.kv_rows(layer) for layer in range(cfg["num_hidden_layers"])]
            _within64(logits, want, f"{name} {n} tokens switch {'on' if on else 'off'}: logits")
            for layer, (got, ref) in enumerate(zip(rows, cache64)):
                for g, r in zip(got, ref):
                    assert g.shape == r.shape and np.abs(g - r).max() <= R64.TOL * max(1.0, np.abs(r).max()), (n, on, layer)
            out[on] = (logits, rows)
        bar = R64.TOL * max(1.0, float(np.abs(want).max()))
        assert float(np.abs(out[True][0].astype(np.float64) - out[False][0]).max()) <= bar
        for a, b in zip(out[True][1], out[False][1]):
            for g, r in zip(a, b):
                assert float(np.abs(g.astype(np.float64) - r).max()) <= R64.TOL * max(1.0, float(np.abs(r).max()))
    long_ones = [i for i, p in enumerate(c.ps) if len(p) >= 24][:6]      # prompts that take the prompt route
    assert len(long_ones) == 6
    for on in (True, False):
        dec.set_fp8_matrix_cores(on)
        assert [dec.generate(c.ps[i], c.news[i]) for i in long_ones] == [c.exp[i] for i in long_ones], on
    dec.set_fp8_matrix_cores(True)


def test_the_switch(fp8_cases, tmp_path):
    from kjarni_amd import HipDecoder
    from kjarni_amd._ffi import KjarniError, KjarniException
    from tests import gguf_fixture as GG
    from tests import synth
    c = fp8_cases("llama-channel")
    dec, ps, news = c.dec, c.ps[:9], c.news[:9]

    def refused(d, word, prompts):
        with pytest.raises(KjarniException) as e:
            d.generate_wide(prompts, 3, lanes=9, lane_context=64)
        assert e.value.code == KjarniError.INVALID_CONFIG and f"more than 8 lanes do not take a {word} {REFUSAL}" in str(e.value), str(e.value)
        with pytest.raises(KjarniException):
            d.wide_begin(9, 64)

    dec.set_fp8_matrix_cores(False)
    assert not dec.fp8_matrix_cores()
    refused(dec, "FP8", ps)
    dec.set_fp8_matrix_cores(True)
    assert dec.generate_wide(ps, news, lanes=9, lane_context=64) == c.exp[:9]
    dec.wide_begin(9, 64)
    dec.set_fp8_matrix_cores(False)                                      # off again: refused, and the wide session is over
    refused(dec, "FP8", ps)
    with pytest.raises(KjarniException):
        dec.wide_step([5] * 9)
    assert dec.generate_wide(ps, news, lanes=8, lane_context=64) == c.exp[:9]
    dec.set_fp8_matrix_cores(True)
    # a GGUF model with the switch on is still refused, and the switch reads back off: the checkpoint is not FP8
    path = str(tmp_path / "q" / "model.gguf")
    qcfg, _ = GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    q = HipDecoder(str(tmp_path / "q"))
    q.set_fp8_matrix_cores(True)
    assert not q.fp8_matrix_cores()
    from tests import lanes_cases as LC
    refused(q, "quantized (GGUF)", LC.prompts(3, qcfg["vocab_size"], n=9))
    # an f32 model: the switch changes nothing, bit for bit
    d = str(tmp_path / "f32")
    fcfg, _ = synth.llm_model(d, synth.LLAMA_TEST, seed=3)
    f = HipDecoder(d, 0)
    ids = np.random.default_rng(2).integers(4, fcfg["vocab_size"], 40).tolist()
    fps = LC.prompts(5, fcfg["vocab_size"], n=12)
    runs = []
    for on in (False, True):
        f.set_fp8_matrix_cores(on)
        assert not f.fp8_matrix_cores()
        f.reset()
        _, logits = f.forward(ids)
        runs.append((logits, f.generate_wide(fps, 5, lanes=12, lane_context=64)))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and runs[0][1] == runs[1][1]


# ---- passengers: what rides behind the pick, one small case each ------------------------------------------------------------------------

def test_logprobs_in_wide_lanes(fp8_cases):
    from tests import sampled_lookup_cases as SC
    from tests.test_gpu_gen_logprobs import _check_records, _raw_rows
    c = fp8_cases("llama-channel")
    ref = SC.Llama64(c.hf, c.cfg)
    ps, news = c.ps[:20], c.news[:20]
    got = c.dec.generate_wide_logprobs(ps, news, top_k=4, lanes=16, lane_context=WF.LANE_CONTEXT)
    assert [g["ids"] for g in got] == c.exp[:20]
    slots = left = 0
    for i, (g, p) in enumerate(zip(got, ps)):
        s, l = _check_records(g, _raw_rows(ref, p, g["ids"]), g["ids"], 4, f"prompt {i}", cap=None)
        slots, left = slots + s, left + l
    assert left <= int(0.02 * slots), f"{left} of {slots} slots left out"


def test_a_pattern_per_lane_equals_the_prompt_alone(fp8_cases):
    from kjarni_amd import constraints as K
    from tests import constraint_cases as CC
    c = fp8_cases("llama-tensor")
    tokens = CC.universal_tokens(c.cfg["vocab_size"], c.cfg["eos_token_id"])
    pats = [K.Constraint(r"(t[0-9]*[02468] )*", tokens), None, K.Constraint(r"(t[12][0-9]* )*", tokens), K.Constraint(r"(.|\n)*", tokens)]
    ps, news = c.ps[:20], c.news[:20]
    autos = [pats[i % 4] for i in range(20)]
    got = c.dec.generate_wide_constrained(ps, news, autos, lanes=16, lane_context=WF.LANE_CONTEXT)
    for i, (g, a) in enumerate(zip(got, autos)):
        if a is None or i % 4 == 3:
            assert g["ids"] == c.exp[i], i
        else:
            ids, _ = c.dec.generate_constrained(a, ps[i], news[i])
            assert g["ids"] == ids and g["result"]["violated"] == 0, i
            assert all((t % 2 == 0) if i % 4 == 0 else str(t)[0] in "12" for t in ids), (i, ids)


def test_prefix_reuse_counters_in_wide_lanes(fp8_cases):
    c = fp8_cases("qwen3-block")
    dec = c.dec
    prefix = np.random.default_rng(77).integers(4, c.cfg["vocab_size"], 24).tolist()
    ps, news = [prefix + p[:12] for p in c.ps[:20]], c.news[:20]
    off = dec.generate_wide(ps, news, lanes=16, lane_context=WF.LANE_CONTEXT)
    assert off == [dec.generate(p, m) for p, m in zip(ps, news)]
    dec.set_prefix_reuse(True)
    try:
        dec.reset()
        r0, c0 = dec.prefix_stats()
        assert dec.generate_wide(ps, news, lanes=16, lane_context=WF.LANE_CONTEXT) == off
        r1, c1 = dec.prefix_stats()
        assert len({p[24] for p in ps}) > 1
        assert c1 - c0 == 24 + sum(len(p) - 24 for p in ps) and r1 - r0 == 24 * len(ps)
    finally:
        dec.set_prefix_reuse(False)


TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


def test_generator_wide_lanes_greedy_and_sampled(tmp_path):
    """Generator.set_wide_lanes + set_fp8_matrix_cores: refused with the switch off; greedy texts equal one by one; a seeded sampled
    run repeats and gives the same texts at widths 16 and 64."""
    from kjarni_amd import Generator
    from kjarni_amd._ffi import KjarniException
    from kjarni_amd.chat import GenerationConfig
    d = str(tmp_path / "gen")
    # (token 188 is the byte 0, which no returned text may hold; a Generator stops on the first eos id of config.json, so as that id
    # it ends a sampled run instead of being emitted)
    F.fp8_model(d, dict(F.QWEN3_F8, vocab_size=720, bos_token_id=700, eos_token_id=[188, 702]), "block", seed=11)
    shutil.copy(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    gen = Generator("qwen3-0.6b", model_path=d)
    texts = [f"{t} {i}" for i in range(14) for t in TEXTS]               # 70 texts: 64 lanes turn over
    greedy = GenerationConfig(do_sample=False, max_new_tokens=8)
    single = [gen.generate(t, greedy) for t in texts[:15]]
    gen.set_wide_lanes(16)
    with pytest.raises(KjarniException) as e:
        gen.generate_batch(texts[:15], greedy)
    assert REFUSAL in str(e.value)
    gen.set_fp8_matrix_cores(True)
    assert gen.generate_batch(texts[:15], greedy) == single
    hot = GenerationConfig(do_sample=True, temperature=1.5, max_new_tokens=8)
    runs = []
    for lanes in (16, 16, 64):
        gen.set_wide_lanes(lanes)
        gen.seed(1234)
        runs.append(gen.generate_batch(texts, hot))
    assert runs[0] == runs[1], "a seeded run does not repeat"
    assert runs[0] == runs[2], "a seeded run differs between widths 16 and 64"
    assert runs[0] != gen.generate_batch(texts, GenerationConfig(do_sample=False, max_new_tokens=8))
    gen.set_fp8_matrix_cores(False)
    gen.set_wide_lanes(0)
    assert gen.generate_batch(texts[:15], greedy) == single


def test_chat_carries_the_switch(tmp_path):
    from kjarni_amd import Chat
    from kjarni_amd.chat import GenerationConfig
    d = str(tmp_path / "chat")
    F.fp8_model(d, dict(F.LLAMA_F8, vocab_size=720, bos_token_id=700, eos_token_id=[701, 704]), "channel", seed=11)
    shutil.copy(os.path.join(GOLDEN, "bpe_llama3_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    chat = Chat("llama3.2-1b-instruct", model_path=d)
    cfg = GenerationConfig(do_sample=False, max_new_tokens=10)
    message = "Is water wet? Answer in one short sentence, and say why you think so."      # a prompt of more than 24 tokens: the prompt route
    plain = chat.send(message, cfg)
    chat.set_fp8_matrix_cores(True)
    assert chat.send(message, cfg) == plain
    chat.set_fp8_matrix_cores(False)
    assert chat.send(message, cfg) == plain
