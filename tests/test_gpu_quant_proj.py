"""The decode step's fused projections alone, mode by mode: launch_qfused (quant_kernels.hip) and launch_fp8_proj
(fp8_kernels.hip) through kjarni_hip_op_fused_proj_ggml / _fp8, and the preparation kernels (qprep, q8k_quantize, qembed), each
against tests/quant_proj_ref64.py at the shapes the whole-model fixtures (hidden 256, intermediate 512) never reach.

Every case pre-fills its outputs, the padding columns of x and the rows of x past `rows` with one NaN bit pattern, and asserts
that every element the operation owns is finite and on the bar and that every other element still holds that pattern.

The bar: 1e-5 x max(1, max |ref|) against float64, the bar of test_gpu_gguf / test_gpu_fp8 for these kernels."""
import itertools

import numpy as np
import pytest

from tests import fp8_fixture as F8
from tests import gguf_fixture as GG
from tests import quant_proj_ref64 as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NAN_BITS = np.uint32(0x7FC01234)
Q8_0, Q4_K, Q6_K = 8, 12, 14
TYPES = (Q8_0, Q4_K, Q6_K)
TNAME = {Q8_0: "Q8_0", Q4_K: "Q4_K", Q6_K: "Q6_K"}
PLAIN, QKV, SWIGLU = 0, 1, 2
CACHE_ROWS = 16


def _ops():
    from kjarni_amd import ops
    return ops


def _refused():
    from kjarni_amd._ffi import KjarniException
    return pytest.raises(KjarniException)


def nans(*shape):
    return np.full(shape, NAN_BITS, np.uint32).view(F32)


def make_x(rng, rows, k, rows_alloc=None, ldx=None, scale=1.0):
    """x [rows_alloc, ldx]: normal of standard deviation `scale` in [:rows, :k], the NaN pattern everywhere else."""
    x = nans(rows_alloc or rows + 1, ldx or k + 8)
    x[:rows, :k] = (scale * rng.standard_normal((rows, k))).astype(F32)
    return x


class Worst:
    """The largest error / bar of a group of cases, printed once."""

    def __init__(self, what):
        self.what, self.ratio, self.err, self.bar, self.case = what, 0.0, 0.0, 0.0, None

    def check(self, got, rows, n, ref, case, row0=0):
        """got [out_rows, ldy]: the operation owns rows row0 .. row0 + rows - 1, columns 0 .. n - 1 and nothing else."""
        own = np.zeros(got.shape, bool)
        own[row0:row0 + rows, :n] = True
        assert (got.view(np.uint32)[~own] == NAN_BITS).all(), f"{self.what} {case}: an element outside the output was written"
        val = got[row0:row0 + rows, :n]
        ref = np.asarray(ref, F64)
        assert val.shape == ref.shape, (val.shape, ref.shape)
        assert np.isfinite(val).all(), f"{self.what} {case}: not finite"
        err, bar = float(np.abs(val - ref).max()), 1e-5 * max(1.0, float(np.abs(ref).max()))
        if err / bar >= self.ratio:
            self.ratio, self.err, self.bar, self.case = err / bar, err, bar, case
        assert err <= bar, f"{self.what} {case}: err {err:.3e} > bar {bar:.3e}"

    def report(self):
        print(f"[quant_proj] {self.what}: largest err {self.err:.3e} (bar {self.bar:.3e}, {self.ratio:.2f} of it) at {self.case}")


# ---- weights, made once ------------------------------------------------------------------------------------------------------------

_CACHE = {}


def ggml_mat(t, n, k, seed=0):
    """(type, blocks, float64 weights) of random_blocks, shared among the tests and never changed."""
    key = ("g", t, n, k, seed)
    if key not in _CACHE:
        b = GG.random_blocks(t, n, k, np.random.default_rng([t, n, k, seed]))
        _CACHE[key] = (t, b, R.ggml_weights64(t, b, n, k))
    return _CACHE[key]


def fp8_mat(kind, n, k, seed=0):
    """(codes, scale [rows, cols], kind, float64 weights) of fp8_fixture.quantize."""
    key = ("f", kind, n, k, seed)
    if key not in _CACHE:
        rng = np.random.default_rng([F8.KINDS.index(kind), n, k, seed])
        codes, scale = F8.quantize(rng.standard_normal((n, k), dtype=F32) * F32(0.05), kind, rng)
        scale = np.ascontiguousarray(scale, F32).reshape(F8.scale_shape(kind, n, k))
        _CACHE[key] = (codes, scale, kind, R.fp8_weights64(codes, scale, kind))
    return _CACHE[key]


def gamma_of(rng, k):
    return (1.0 + 0.1 * rng.standard_normal(k)).astype(F32)


def norm64(x, rows, k, gamma, eps):
    xr = x[:rows, :k].astype(F64)
    return xr if gamma is None else R.rms_norm64(xr, gamma, eps)


# ---- 1. position probes, bit for bit ---------------------------------------------------------------------------------------------

def _probe_positions(k, slice_cols):
    pos = {0, 15, 16, min(slice_cols, k) - 1, k - 1}
    for s in range(1, (k + slice_cols - 1) // slice_cols):
        pos |= {s * slice_cols, min((s + 1) * slice_cols, k) - 1}
    return sorted(p for p in pos if 0 <= p < k)


def _fp8_probe_matrix(kind, n, k):
    rng = np.random.default_rng([7, F8.KINDS.index(kind), k])
    codes, scale = F8.quantize(rng.standard_normal((n, k), dtype=F32) * F32(0.05), kind, rng)
    codes = np.where((codes & 0x7F) == 0, np.uint8(0x38), codes).astype(np.uint8)      # no zero weight: every probe tells a scale apart
    shape = F8.scale_shape(kind, n, k)
    if kind == "block":      # a distinct power of two per 128 x 128 tile: another tile's scale changes the bits
        scale = np.exp2(np.arange(shape[0] * shape[1], dtype=F64) - 60.0).astype(F32)
    scale = np.ascontiguousarray(scale, F32).reshape(shape)
    return codes, scale, F8.dequantize(codes, scale, kind)


@pytest.mark.parametrize("kind", F8.KINDS)
def test_fp8_position_probes_are_bit_exact(kind):
    """x one-hot, one position per row: y[r, j] is the f32 dequantized w[j, pos_r], exactly (plain mode, no norm)."""
    ops, n = _ops(), 22
    blk = kind == "block"
    one_row = [2048, 8192, 2176 if blk else 2064, 8320 if blk else 8208, 14336]
    eight = [128, 2048, 2176 if blk else 2064, 6144]
    for rows, ks in ((1, one_row), (8, eight)):
        for k in ks:
            codes, scale, w = _fp8_probe_matrix(kind, n, k)
            pos = _probe_positions(k, 8192 if rows == 1 and k > 2048 else 2048)
            pos += [p for p in (k // 2 + 3, k // 4 + 1, 1, k - 17, 33, 64, 100, 2) if p not in pos][:(-len(pos)) % rows]
            for c in range(0, len(pos), rows):
                chunk = pos[c:c + rows]
                x = nans(rows + 1, k + 4)
                x[:rows, :k] = 0.0
                x[np.arange(rows), chunk] = 1.0
                (y,) = ops.fused_proj_fp8(PLAIN, [(codes, scale)], x, rows, [nans(rows, n + 3)])
                assert (y.view(np.uint32)[:, n:] == NAN_BITS).all()
                for r, p in enumerate(chunk):
                    assert np.array_equal(y[r, :n], w[:, p]), (kind, rows, k, p, y[r, :n], w[:, p])


@pytest.mark.parametrize("t", TYPES, ids=[TNAME[t] for t in TYPES])
def test_ggml_position_probes_are_bit_exact(t):
    ops, n = _ops(), 6
    for k in (256, 2048, 2304, 4352):
        _, blocks, _ = ggml_mat(t, n, k, seed=1)
        w = GG.dequantize(t, blocks, n, k)
        pos = sorted({p for p in (0, 31, 32, 255, 256, k - 1) if p < k})
        last = (k // 256 - 1) * 256
        pos += [last + 32 * g + (5 * g + 3) % 32 for g in range(8)]      # one position in each 32-group of the last 256-block
        for rows in (8, 1):
            use = pos if rows == 8 else [pos[-1], k - 1]
            use = use + [p for p in (1, 17, 100, 200, 77, 130, 250) if p not in use][:(-len(use)) % rows]
            for c in range(0, len(use), rows):
                chunk = use[c:c + rows]
                x = nans(rows + 1, k + 4)
                x[:rows, :k] = 0.0
                x[np.arange(rows), chunk] = 1.0
                (y,), _ = ops.fused_proj_ggml(PLAIN, [(t, blocks)], x, rows, [nans(rows, n + 3)], k=k)
                assert (y.view(np.uint32)[:, n:] == NAN_BITS).all()
                for r, p in enumerate(chunk):
                    assert np.array_equal(y[r, :n], w[:, p]), (TNAME[t], rows, k, p, y[r, :n], w[:, p])


# ---- 2. the wide FP8 instances (>= 8 177 columns, more than one row) -----------------------------------------------------------

def _fp8_run(worst, case, mode, mats, rng, rows, k, gamma=False, bias=False, resid=None, row_off=0, on_device=False, eps=1e-5,
             push=None):
    """One launch_fp8_proj against float64.  mats: fp8_mat() tuples.  resid: None, "apart" or "in_place".  push: (column, target)
    -- SwiGLU: gamma scaled so that row 0's gate sum of that column is `target`."""
    ops = _ops()
    ns = [m[0].shape[0] for m in mats]
    x = make_x(rng, rows, k, rows_alloc=rows + 2, scale=0.01 if gamma and rows in (3, 8) else 1.0)      # small rows: eps carries weight
    g = gamma_of(rng, k) if gamma else None
    if push is not None:
        col, target = push
        sign = np.sign(mats[0][3][col])
        for r in range(rows):
            x[r, :k] = ((1.0 if r % 2 == 0 else -1.0) * sign + 0.1 * rng.standard_normal(k)).astype(F32)
        g = (g.astype(F64) * (target / float(norm64(x, 1, k, g, eps)[0] @ mats[0][3][col]))).astype(F32)
    n_tot = ns[0] if mode == SWIGLU else sum(ns)
    b = (0.5 * rng.standard_normal(n_tot) + np.arange(n_tot) * 1e-3).astype(F32) if bias else None
    xn = norm64(x, rows, k, g, eps)
    prods = [xn @ m[3].T for m in mats]
    bsplit = None if b is None else ([b] if mode == SWIGLU else [b[sum(ns[:i]):sum(ns[:i + 1])] for i in range(len(ns))])
    if mode == QKV:
        ys = [nans(rows + 1, ns[0] + 5), nans(CACHE_ROWS, ns[1] + 3), nans(CACHE_ROWS, ns[2] + 1)]
    else:
        ys = [nans(rows + 1, ns[0] + 5)]
    rmat, r_apart = None, None
    if resid:
        rmat = rng.standard_normal((rows, ns[0])).astype(F32)
        if resid == "in_place":
            ys[0][:rows, :ns[0]] = rmat
        else:
            r_apart = nans(rows, ns[0] + 7)
            r_apart[:, :ns[0]] = rmat
    want = R.finish64("swiglu" if mode == SWIGLU else "plain", prods, bsplit, rmat)
    got = ops.fused_proj_fp8(mode, [(m[0], m[1]) for m in mats], x, rows, ys, gamma=g, eps=eps, bias=b, r=r_apart,
                             r_is_y0=resid == "in_place", row_off=row_off, offset_on_device=on_device)
    for i, (gy, wy) in enumerate(zip(got, want)):
        worst.check(gy, rows, ns[0] if mode == SWIGLU else ns[i], wy, f"{case} out{i}", row0=0 if i == 0 else row_off)


@pytest.mark.parametrize("kind", F8.KINDS)
def test_fp8_wide_plain(kind):
    worst = Worst(f"fp8 wide plain {kind}")
    rng = np.random.default_rng(11)
    for k in (128, 2176):
        m = fp8_mat(kind, 8200, k)
        for rows in (2, 8):
            _fp8_run(worst, f"k={k} rows={rows}", PLAIN, [m], rng, rows, k, bias=rows == 8)
    worst.report()


@pytest.mark.parametrize("kinds", [("tensor",) * 3, ("channel",) * 3, ("block",) * 3, ("block", "channel", "tensor")],
                         ids=["tensor", "channel", "block", "mixed"])
def test_fp8_wide_qkv_boundaries_inside_a_wave(kinds):
    """A wave of the four-columns instance owns columns n0 .. n0 + 3 with n0 a multiple of 4.  6146 | 1027 | 1027 puts the
    boundaries at 6146 and 7173: the wave of 6144 .. 6147 holds two columns of Q and two of K, the wave of 7172 .. 7175 one of K
    and three of V, so one wave picks two segments' rows, scales and outputs.  6144 | 1028 | 1028 (the sizes first asked for) has
    both boundaries on a multiple of 4, between two waves: kept as the aligned case beside it."""
    rng = np.random.default_rng(12)
    k = 256
    for sizes in ((6146, 1027, 1027), (6144, 1028, 1028)):
        worst = Worst(f"fp8 wide qkv {'/'.join(kinds)} {sizes[0]}|{sizes[1]}|{sizes[2]}")
        mats = [fp8_mat(kd, n, k, seed=i) for i, (kd, n) in enumerate(zip(kinds, sizes))]
        for rows, off, dev in ((2, 5, True), (8, 8, False)):
            _fp8_run(worst, f"rows={rows}", QKV, mats, rng, rows, k, gamma=True, bias=True, row_off=off, on_device=dev)
        worst.report()


@pytest.mark.parametrize("kinds", [("tensor", "tensor"), ("channel", "channel"), ("block", "block"), ("block", "channel")],
                         ids=["tensor", "channel", "block", "mixed"])
def test_fp8_wide_swiglu(kinds):
    worst = Worst(f"fp8 wide swiglu {'/'.join(kinds)}")
    rng = np.random.default_rng(13)
    k = 256
    mats = [fp8_mat(kd, 8200, k, seed=10 + i) for i, kd in enumerate(kinds)]
    for rows in (2, 8):
        _fp8_run(worst, f"rows={rows}", SWIGLU, mats, rng, rows, k, gamma=True)
    worst.report()


# ---- 3. every mode, FP8 --------------------------------------------------------------------------------------------------------

ROWS = (1, 3, 5, 8)


def _offsets(rows):
    return (0, 5, CACHE_ROWS - rows)


@pytest.mark.parametrize("kinds", [("tensor",) * 3, ("channel",) * 3, ("block",) * 3, ("channel", "tensor", "block")],
                         ids=["tensor", "channel", "block", "mixed"])
def test_fp8_qkv_every_option(kinds):
    worst = Worst(f"fp8 qkv {'/'.join(kinds)}")
    rng = np.random.default_rng(21)
    i = 0
    for k in (256, 2304):      # one slice; two slices (rows > 1) with a part-full last one
        mats = [fp8_mat(kd, n, k, seed=20 + j) for j, (kd, n) in enumerate(zip(kinds, (200, 72, 42)))]
        for rows in ROWS:
            for off in _offsets(rows):
                _fp8_run(worst, f"k={k} rows={rows} off={off}", QKV, mats, rng, rows, k, gamma=i % 2 == 0, bias=i % 3 != 2, row_off=off,
                         on_device=(i // 2) % 2 == 0)
                i += 1
    # every offset at every row count, by value and on the device, with and without the norm, on one geometry
    mats = [fp8_mat(kd, n, 256, seed=20 + j) for j, (kd, n) in enumerate(zip(kinds, (200, 72, 42)))]
    for rows in ROWS:
        for off in _offsets(rows):
            for dev in (False, True):
                for gamma in (False, True):
                    _fp8_run(worst, f"rows={rows} off={off} dev={int(dev)} norm={int(gamma)}", QKV, mats, rng, rows, 256, gamma=gamma, bias=True,
                             row_off=off, on_device=dev)
    worst.report()


@pytest.mark.parametrize("kinds", list(itertools.product(F8.KINDS, F8.KINDS)), ids=lambda p: "-".join(p))
def test_fp8_swiglu_pairs_and_a_saturated_gate(kinds):
    worst, pushed = Worst(f"fp8 swiglu {'/'.join(kinds)}"), Worst(f"fp8 swiglu {'/'.join(kinds)}, gate at +-90")
    rng = np.random.default_rng(22)
    k, n = 384, 201
    mats = [fp8_mat(kd, n, k, seed=30 + j) for j, kd in enumerate(kinds)]
    for rows in ROWS:
        _fp8_run(worst, f"rows={rows}", SWIGLU, mats, rng, rows, k, gamma=True)
        _fp8_run(pushed, f"rows={rows}", SWIGLU, mats, rng, rows, k, gamma=True, push=(n - 1, 90.0))
    worst.report()
    pushed.report()


@pytest.mark.parametrize("kind", F8.KINDS)
def test_fp8_residual_on_the_multi_slice_path(kind):
    """K = 14 336 with one row (two slices of the CH = 8 instance) and K = 6 144 with five rows (three slices), R apart from Y with
    ldr > n and R as Y in place; one slice for comparison.  K = 14 336 is beyond the K <= 8 192 the bar was stated for; measured there:
    5.9e-6 against a bar of 1.8e-4, so the bar stands as it is."""
    worst = Worst(f"fp8 residual {kind}")
    rng = np.random.default_rng(23)
    for k, rows in ((14336, 1), (6144, 5), (256, 3)):
        m = fp8_mat(kind, 203, k, seed=40)
        for resid in ("apart", "in_place"):
            _fp8_run(worst, f"k={k} rows={rows} {resid}", PLAIN, [m], rng, rows, k, bias=resid == "apart", resid=resid)
    worst.report()


@pytest.mark.parametrize("kind", F8.KINDS)
def test_fp8_norm_with_several_slices(kind):
    worst = Worst(f"fp8 norm + slices {kind}")
    rng = np.random.default_rng(24)
    for k, rows in ((4096, 8), (2176, 8), (8320, 1), (14336, 1)):
        qkv = [fp8_mat(kind, n, k, seed=50 + j) for j, n in enumerate((72, 40, 24))]
        _fp8_run(worst, f"qkv k={k} rows={rows}", QKV, qkv, rng, rows, k, gamma=True, bias=True, row_off=3, on_device=True)
        sw = [fp8_mat(kind, 100, k, seed=60 + j) for j in range(2)]
        _fp8_run(worst, f"swiglu k={k} rows={rows}", SWIGLU, sw, rng, rows, k, gamma=True)
    worst.report()


# ---- 4. every mode, GGUF -------------------------------------------------------------------------------------------------------

def _q8k_checks(worst, case, x, rows, k, g, eps, q8k_out):
    """The device's normalised rows against float64, and its codes / scales against the f32 restatement on those rows, exactly."""
    xn, xq, xd = q8k_out
    src = x[:rows, :k]
    if g is not None:
        worst.check(xn, rows, k, R.rms_norm64(src.astype(F64), g, eps), f"{case} xn")
        src = xn
    q, d = GG.q8k_quantize(src)
    assert np.array_equal(xq.astype(np.int32), q) and np.array_equal(xd, d), f"{case}: Q8_K codes differ from the restatement"
    return xq, xd


def _ggml_run(worst, case, mode, mats, rng, rows, k, gamma=False, bias=False, resid=None, row_off=0, on_device=False, eps=1e-5,
              q8k=False, head_dim=0, push=None):
    """One launch_qfused against float64.  mats: ggml_mat() tuples."""
    ops = _ops()
    ns = [m[1].shape[0] for m in mats]
    x = make_x(rng, rows, k, rows_alloc=rows + 2, scale=0.01 if gamma and rows in (3, 8) else 1.0)      # small rows: eps carries weight
    g = gamma_of(rng, k) if gamma else None
    if push is not None:
        col, target = push
        sign = np.sign(mats[0][2][col])
        for r in range(rows):
            x[r, :k] = ((1.0 if r % 2 == 0 else -1.0) * sign + 0.1 * rng.standard_normal(k)).astype(F32)
        g = (g.astype(F64) * (target / float(norm64(x, 1, k, g, eps)[0] @ mats[0][2][col]))).astype(F32)
    b, boff, bsplit = None, (0, 0, 0), None
    if bias:      # segments anywhere in the bias buffer, in another order than the matrices
        gap = (3, 2, 5)
        order = (2, 0, 1)[:len(ns)] if mode == QKV else (0,)
        boff, at = [0, 0, 0], 0
        for s in order:
            at += gap[s]
            boff[s] = at
            at += ns[s]
        b = (0.5 * rng.standard_normal(at + 4) + np.arange(at + 4) * 1e-3).astype(F32)
        bsplit = [b[boff[s]:boff[s] + ns[s]] for s in range(1 if mode != QKV else 3)]
    rope = None
    if mode == QKV:
        ang = rng.uniform(-np.pi, np.pi, (CACHE_ROWS, head_dim // 2))
        rope = dict(head_dim=head_dim, cos=np.cos(ang).astype(F32), sin=np.sin(ang).astype(F32), off=row_off)
        ys = [nans(rows + 1, ns[0] + 5), nans(CACHE_ROWS, ns[1] + 3), nans(CACHE_ROWS, ns[2] + 1)]
    else:
        ys = [nans(rows + 1, ns[0] + 5)]
    rmat, r_apart = None, None
    if resid:
        rmat = rng.standard_normal((rows, ns[0])).astype(F32)
        if resid == "in_place":
            ys[0][:rows, :ns[0]] = rmat
        else:
            r_apart = nans(rows, ns[0] + 7)
            r_apart[:, :ns[0]] = rmat
    got, q8k_out = ops.fused_proj_ggml(mode, [(m[0], m[1]) for m in mats], x, rows, ys, gamma=g, eps=eps, bias=b, bias_off=boff, r=r_apart,
                                       r_is_y0=resid == "in_place", row_off=row_off, offset_on_device=on_device, head_dim=head_dim,
                                       cos=None if rope is None else rope["cos"], sin=None if rope is None else rope["sin"], q8k=q8k, k=k)
    codes = _q8k_checks(worst, case, x, rows, k, g, eps, q8k_out) if q8k else None
    xn = norm64(x, rows, k, g, eps)
    prods = [R.ggml_product64(xn, m[0], m[1], n, k, codes) if m[0] == Q6_K and q8k else xn @ m[2].T for m, n in zip(mats, ns)]
    if mode == QKV:
        want = R.finish64("qkv", prods, bsplit, None, rope)
    else:
        want = R.finish64("swiglu" if mode == SWIGLU else "plain", prods, bsplit, rmat)
    for i, (gy, wy) in enumerate(zip(got, want)):
        worst.check(gy, rows, ns[0] if mode == SWIGLU else ns[i], wy, f"{case} out{i}", row0=0 if i == 0 else row_off)


ROTATIONS = [(Q4_K, Q8_0, Q6_K), (Q8_0, Q6_K, Q4_K), (Q6_K, Q4_K, Q8_0)]


@pytest.mark.parametrize("q8k", [False, True], ids=["f32", "q8k"])
@pytest.mark.parametrize("rot", range(3), ids=["-".join(TNAME[t] for t in r) for r in ROTATIONS])
def test_ggml_qkv_every_option(rot, q8k):
    """head_dim 8 / 64 / 128 on the decoder's geometry, heads x head_dim = H = K = 256, for every rotation of the types; then one
    geometry crossed with every offset, whose K (256, 2304, 512 by rotation) is not the width of Q: the kernel does not tie n to
    k, and 2304 gives the part-filled last step."""
    types = ROTATIONS[rot]
    worst = Worst(f"ggml qkv {'/'.join(TNAME[t] for t in types)} q8k={int(q8k)}")
    rng = np.random.default_rng(31 + rot)
    k = 256
    i = rot
    for head_dim, heads, kv_heads in ((8, 32, 3), (64, 4, 2), (128, 2, 1)):
        mats = [ggml_mat(t, n, k, seed=70 + j) for j, (t, n) in enumerate(zip(types, (heads * head_dim, kv_heads * head_dim, kv_heads * head_dim)))]
        for rows in ROWS:
            off = _offsets(rows)[i % 3]
            _ggml_run(worst, f"d={head_dim} rows={rows} off={off}", QKV, mats, rng, rows, k, gamma=i % 2 == 0, bias=i % 4 != 3, row_off=off,
                      on_device=(i // 2) % 2 == 0, q8k=q8k, head_dim=head_dim)
            i += 1
    # every offset at every row count, by value and on the device, on one geometry
    k = (256, 2304, 512)[rot]
    mats = [ggml_mat(t, n, k, seed=80 + j) for j, (t, n) in enumerate(zip(types, (128, 64, 64)))]
    for rows in ROWS:
        for off in _offsets(rows):
            for dev in (False, True):
                _ggml_run(worst, f"d=64 rows={rows} off={off} dev={int(dev)}", QKV, mats, rng, rows, k, gamma=True, bias=True, row_off=off,
                          on_device=dev, q8k=q8k, head_dim=64)
    worst.report()


@pytest.mark.parametrize("pair", list(itertools.product(TYPES, TYPES)), ids=lambda p: "-".join(TNAME[t] for t in p))
def test_ggml_swiglu_pairs_and_a_saturated_gate(pair):
    """Same-type pairs take the paired route of qpair, mixed pairs the one-column-at-a-time route."""
    name = "/".join(TNAME[t] for t in pair)
    worst, pushed = Worst(f"ggml swiglu {name}"), Worst(f"ggml swiglu {name}, gate at +-90")
    rng = np.random.default_rng(32)
    k, n = 2304, 37
    mats = [ggml_mat(t, n, k, seed=90 + j) for j, t in enumerate(pair)]
    for i, rows in enumerate(ROWS):
        q8k = Q6_K in pair and i % 2 == 0
        _ggml_run(worst, f"rows={rows} q8k={int(q8k)}", SWIGLU, mats, rng, rows, k, gamma=True, q8k=q8k)
        _ggml_run(pushed, f"rows={rows}", SWIGLU, mats, rng, rows, k, gamma=True, push=(n - 1, 90.0 if i % 2 == 0 else -90.0))
    worst.report()
    pushed.report()


@pytest.mark.parametrize("t", TYPES, ids=[TNAME[t] for t in TYPES])
def test_ggml_residual_bias_and_odd_n(t):
    """n = 1 and 201: the lone last column of qfused_kernel / qpair (two == false); 200 for the paired form.  R apart from Y
    with ldr > n, and R as Y in place."""
    worst = Worst(f"ggml residual / odd n {TNAME[t]}")
    rng = np.random.default_rng(33)
    i = 0
    for k in (256, 2304):
        for n in (1, 201, 200):
            m = ggml_mat(t, n, k, seed=100)
            for rows in ROWS:
                for resid in ("apart", "in_place"):
                    _ggml_run(worst, f"k={k} n={n} rows={rows} {resid}", PLAIN, [m], rng, rows, k, bias=i % 3 != 2, resid=resid,
                              q8k=t == Q6_K and i % 2 == 0, gamma=t != Q6_K and i % 4 == 1)
                    i += 1
    worst.report()


# ---- 5. the preparation kernels alone ----------------------------------------------------------------------------------------

def _q8k_input(rng, rows, k, ldx):
    """Rows within 1e-3 <= |x| <= 1e3 or exactly 0; block 0 of row 0 all zero (when there is another block to keep the row
    alive), the last block of the last row scaled to amax = 127 with exact ties."""
    x = nans(rows, ldx)
    mag = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (rows, k)))
    x[:, :k] = (mag * rng.choice([-1.0, 1.0], (rows, k))).astype(F32)
    x[:, :k][rng.random((rows, k)) < 0.02] = 0.0
    if rows * k > 256:
        x[0, :256] = 0.0
    tie = rng.integers(-126, 127, 256).astype(F32)
    tie[:8] = (0.5, -0.5, 2.5, -2.5, 126.5, -126.5, 127.0, 1.5)
    x[rows - 1, k - 256:k] = tie
    return x


@pytest.mark.parametrize("rows,k", [(1, 256), (1, 2304), (8, 256), (8, 2304)])
def test_q8k_quantize_and_qprep_equal_the_f32_restatement(rows, k):
    ops = _ops()
    rng = np.random.default_rng([41, rows, k])
    x = _q8k_input(rng, rows, k, k + 12)
    q, d, deq = R.q8k_f32(x[:, :k])
    if rows * k > 256:
        assert (q[0, :256] == 0).all() and d[0, 0] == 0.0                        # the zero block: d = 0, codes 0
    assert d[rows - 1, -1] == 1.0 and q[rows - 1, k - 256:k - 248].tolist() == [1, -1, 3, -3, 127, -127, 127, 2]   # ties away from zero
    codes, scales, dq = ops.q8k_quantize(x, k)
    assert np.array_equal(codes.astype(np.int32), q) and np.array_equal(scales, d) and np.array_equal(dq, deq)
    # qprep without gamma: the same codes from the rows as they are (then a Q6_K launch on them)
    m = ggml_mat(Q6_K, 3, k, seed=110)
    xa = nans(rows + 1, k + 12)
    xa[:rows] = x
    (y,), (xn, xq, xd) = ops.fused_proj_ggml(PLAIN, [(m[0], m[1])], xa, rows, [nans(rows, 3)], q8k=True, k=k)
    assert np.array_equal(xq.astype(np.int32), q) and np.array_equal(xd, d)
    assert (xn.view(np.uint32) == np.full(1, np.nan, F32).view(np.uint32)[0]).all()      # no gamma: no normalised rows
    worst = Worst(f"qprep rows={rows} k={k}")
    worst.check(y, rows, 3, R.q6k_on_codes64(xq, xd, m[1], 3, k), "Q6_K on the codes")
    # qprep with gamma: xn against float64, its codes exactly those of the device's xn
    xs = make_x(rng, rows, k, rows_alloc=rows + 1, ldx=k + 12, scale=0.01)      # mean(x^2) = 1e-4: eps carries weight
    g = gamma_of(rng, k)
    _, out = ops.fused_proj_ggml(PLAIN, [(m[0], m[1])], xs, rows, [nans(rows, 3)], gamma=g, eps=1e-5, q8k=True, k=k)
    _q8k_checks(worst, "norm", xs, rows, k, g, 1e-5, out)
    worst.report()


@pytest.mark.parametrize("t", TYPES, ids=[TNAME[t] for t in TYPES])
def test_qembed_rows_are_the_dequantized_rows_or_zeros(t):
    ops = _ops()
    vocab = 37
    for k in (256, 2304):
        _, blocks, _ = ggml_mat(t, vocab, k, seed=120)
        w = GG.dequantize(t, blocks, vocab, k)
        ids = np.array([0, vocab - 1, vocab, 0xFFFFFFFF, 5, vocab + 1, 0x80000000, 36, 1], np.uint32)
        out = ops.qembed(ids, t, blocks, vocab, k)
        for i, tok in enumerate(ids):
            want = w[tok] if tok < vocab else np.zeros(k, F32)
            assert np.array_equal(out[i], want), (TNAME[t], k, int(tok))


# ---- 6. refusals: an error, and the outputs as they were ---------------------------------------------------------------------

def _fp8_call(rows=2, k=256, n=(24,), mode=PLAIN, ldx=None, gamma=False, r=False, out_rows=12, row_off=0, **kw):
    """A small per-tensor call (every weight 1.0); returns (the call, its outputs, which it writes in place)."""
    ops = _ops()
    pairs = [(np.full((nn, k), 0x38, np.uint8), np.ones((1, 1), F32)) for nn in n]
    x = np.ones((max(rows, 1) + 1, ldx or k), F32)
    ys = [nans(out_rows, nn) for nn in (n if mode == QKV else n[:1])]
    g = np.ones(k, F32) if gamma else None
    rr = np.ones((max(rows, 1), n[0]), F32) if r else None
    return (lambda: ops.fused_proj_fp8(mode, pairs, x, rows, ys, gamma=g, eps=1e-5, r=rr, row_off=row_off, in_place=True, **kw)), ys


def _untouched(ys):
    return all((y.view(np.uint32) == NAN_BITS).all() for y in ys)


def test_fp8_refusals_leave_the_outputs_untouched():
    ok, ys = _fp8_call()
    ok()
    assert not _untouched(ys)      # the same call with nothing wrong runs
    cases = dict(
        swiglu_without_gamma=dict(mode=SWIGLU, n=(24, 24)),
        swiglu_with_r=dict(mode=SWIGLU, n=(24, 24), gamma=True, r=True),
        r_with_gamma=dict(gamma=True, r=True),
        gate_up_different_n=dict(mode=SWIGLU, n=(24, 40), gamma=True),
        rows_0=dict(rows=0), rows_9=dict(rows=9),
        ldx_not_4=dict(ldx=258),
        k_not_16=dict(k=248, ldx=256),
        capacity=dict(mode=QKV, n=(24, 8, 8), out_rows=12, row_off=11),
        capacity_on_device=dict(mode=QKV, n=(24, 8, 8), out_rows=12, row_off=11, offset_on_device=True),
        negative_offset=dict(mode=QKV, n=(24, 8, 8), row_off=-1),
    )
    for name, kw in cases.items():
        call, ys = _fp8_call(**kw)
        with _refused():
            call()
        assert _untouched(ys), name
    # block scales need k % 128 == 0: [ceil(n / 128), k / 128] fits no k = 144
    ops = _ops()
    ys = [nans(3, 24)]
    with _refused():
        ops.fused_proj_fp8(PLAIN, [(np.zeros((24, 144), np.uint8), np.ones((1, 2), F32))], np.ones((3, 144), F32), 2, ys, in_place=True)
    assert _untouched(ys)


def test_ggml_refusals_leave_the_outputs_untouched():
    ops = _ops()
    t, blocks, _ = ggml_mat(Q8_0, 24, 256, seed=140)
    kvb = ggml_mat(Q8_0, 8, 256, seed=141)[1]
    tab = np.ones((12, 4), F32)

    def call(rows=2, k=256, mode=PLAIN, out_rows=12, row_off=0, tab_rows=12, **kw):
        bl = blocks if k == 256 else GG.random_blocks(Q8_0, 24, k, np.random.default_rng(0))
        mats = [(t, bl)] + ([(t, kvb), (t, kvb)] if mode == QKV else [])
        ys = [nans(out_rows, 24)] + ([nans(out_rows, 8), nans(out_rows, 8)] if mode == QKV else [])
        extra = dict(head_dim=8, cos=tab[:tab_rows], sin=tab[:tab_rows]) if mode == QKV else {}
        return (lambda: ops.fused_proj_ggml(mode, mats, np.ones((max(rows, 1) + 1, k), F32), rows, ys, row_off=row_off, k=k, in_place=True,
                                            **extra, **kw)), ys
    ok, ys = call(mode=QKV, row_off=10)
    ok()
    assert not _untouched(ys)
    for name, kw in dict(rows_0=dict(rows=0), rows_9=dict(rows=9), k_not_256=dict(k=288),
                         capacity=dict(mode=QKV, row_off=11), capacity_on_device=dict(mode=QKV, row_off=11, offset_on_device=True),
                         position=dict(mode=QKV, row_off=9, tab_rows=10), position_on_device=dict(mode=QKV, row_off=9, tab_rows=10, offset_on_device=True),
                         bias_off=dict(bias=np.ones(24, F32), bias_off=(1, 0, 0))).items():
        c, ys = call(**kw)
        with _refused():
            c()
        assert _untouched(ys), name
