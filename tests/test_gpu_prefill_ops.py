"""The prompt route's four kernels alone -- prefill_gemm_kernel / prefill_gemm_bf16w_kernel with prefill_splitk_reduce_kernel, and
prefill_attention_kernel / prefill_attention_mfma_kernel -- through kjarni_hip_op_prefill_gemm / _prefill_attention, against the
float64 references of tests/prefill_ref64.py and tests/decode_attention_ref64.py.

Inputs are standard normal.  Everything a kernel may over-read but must not use is NaN beforehand (A's rows behind m and its
padding columns, K / V rows behind base + rows and their padding columns, q's padding, the split scratch) and the result must be
finite; the padding columns of Y and ctx hold a sentinel that must survive bit for bit.  Bars: the projections 1e-5 * max(1,
max |ref|) (the linear tests' bar; bf16 weights are widened exactly in the reference), the context 1e-5 absolute (a convex
combination of O(1) values).  Every comparison goes through tests.parity_report."""
import numpy as np
import pytest

from kjarni_amd import ops
from tests import decode_attention_ref64 as R
from tests import prefill_ref64 as P
from tests.parity_report import report

pytestmark = pytest.mark.gpu

TOL = 1e-5
SENTINEL = np.float32(-777.25)
WEIGHTS = [False, True]
WIDS = ["f32", "bf16"]


# ---- the GEMM -------------------------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _gemm_inputs(seed, m, n, k, bf16, pad_a=0):
    rng = np.random.default_rng(seed)
    a = np.full((m + 3, k + pad_a), np.nan, np.float32)
    a[:m, :k] = rng.standard_normal((m, k)).astype(np.float32)
    w = rng.standard_normal((n, k)).astype(np.float32)
    return rng, a, (ops.to_bf16(w) if bf16 else w)


def _check_gemm(name, got, ref):
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), "the result holds NaN / inf: an over-read row, padding or the scratch's poison was used"
    bar = TOL * max(1.0, float(np.abs(ref).max()))
    err = report(name, np.abs(got - ref).max(), bar)
    print(f"{name}: max |kernel - float64| = {err:.3e} (bar {bar:.3e})")
    assert err < bar, err
    return err


def _gemm(name, seed, m, n, k, bf16, split=True, epilogue="none", pad_a=0, pad_y=0, want_ksplit=None):
    """One call with the epilogue named, checked against float64; returns (y[:, :n] or the folded gate, ksplit_used)."""
    rng, a, w = _gemm_inputs(seed, m, n, k, bf16, pad_a)
    bias = rng.standard_normal(n).astype(np.float32) if epilogue in ("bias", "bias+inplace") else None
    y = np.full((m, n + pad_y), SENTINEL, np.float32)
    r = r_ref = gate = None
    if epilogue == "residual":                                           # a buffer of its own, wider than n: ldr > ldy
        r = np.full((m, n + 8), np.nan, np.float32)
        r[:, :n] = rng.standard_normal((m, n)).astype(np.float32)
        r_ref = r[:, :n]
    elif epilogue in ("inplace", "bias+inplace"):
        y[:, :n] = rng.standard_normal((m, n)).astype(np.float32)
        r_ref = y[:, :n].copy()
    elif epilogue == "gate":
        gate = rng.standard_normal((m, n)).astype(np.float32)
    y_before = y.copy()
    out = ops.prefill_gemm(a, w, m, y, bias=bias, r=r, r_is_y=epilogue in ("inplace", "bias+inplace"), gate=gate, bf16=bf16, split=split,
                           want_scratch_written=split)
    got_y, got_g, used = out[0], out[1], out[2]
    want = P.ksplit_rule(m, n, k, split) if want_ksplit is None else want_ksplit
    assert used == want, (used, want)
    if split:  # every partial tile element written once, nothing else touched; unsplit launches leave the scratch alone
        assert out[3] == (used * m * n if used > 1 else 0), (out[3], used, m, n)
    assert np.array_equal(_bits(got_y[:, n:]), _bits(y_before[:, n:])), "the padding columns of Y were written"
    if epilogue == "gate":
        ref_y, ref_g = P.gemm64(a[:m, :k], w, gate=gate, bf16=bf16)
        _check_gemm(name + " fold", got_g, ref_g)
        if used > 1:   # the reduce kernel folds the product into the gate buffer and leaves Y as it was
            assert np.array_equal(_bits(got_y), _bits(y_before))
        else:          # launch_swiglu_mul reads the product from Y
            _check_gemm(name + " product", got_y[:, :n], ref_y)
        return got_g, used
    _check_gemm(name, got_y[:, :n], P.gemm64(a[:m, :k], w, bias, r_ref, bf16=bf16))
    return got_y[:, :n], used


TABLE = [
    (24, 64, 32, 1), (63, 60, 96, 1), (64, 64, 192, 1), (65, 68, 256, 2), (100, 132, 320, 2), (33, 64, 512, 4), (70, 196, 768, 4),
    (64, 128, 1024, 8), (65, 132, 1280, 8), (1, 4, 1024, 8), (129, 64, 1024, 8), (65, 4160, 1024, 4), (65, 16448, 256, 1), (24, 37, 1024, 1),
]


@pytest.mark.parametrize("bf16", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("m,n,k,ksplit", TABLE, ids=lambda v: str(v))
def test_gemm_table(m, n, k, ksplit, bf16):
    """Every split the rule can give, the tile cap that pulls 8 back to 4, the cap above 512 tiles and n % 4 (both with the scratch
    given and found all NaN afterwards), ragged tiles, one row, odd and single K-tile counts."""
    _gemm(f"prefill_gemm {WIDS[bf16]} {m}x{n}x{k}", 1000 + m + n + k, m, n, k, bf16, want_ksplit=ksplit)


EPILOGUES = ["bias", "residual", "inplace", "bias+inplace", "gate"]
EPI_SHAPES = [(65, 68, 256), (70, 196, 768), (64, 128, 1024)]


@pytest.mark.parametrize("bf16", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("m,n,k", EPI_SHAPES, ids=lambda v: str(v))
def test_gemm_epilogues(m, n, k, epilogue, split, bf16):
    """Bias, a residual of its own with ldr > n, the residual in place, both, and the SwiGLU fold: in the reduce kernel (split) and in
    the tile kernel's own epilogue or launch_swiglu_mul (unsplit)."""
    _, used = _gemm(f"prefill_gemm {WIDS[bf16]} {m}x{n}x{k} {epilogue} {'split' if split else 'unsplit'}", 2000 + m + n + k, m, n, k, bf16,
                    split=split, epilogue=epilogue)
    assert (used > 1) == split


@pytest.mark.parametrize("bf16", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("m,n,k,epilogue", [(63, 60, 96, "bias"), (65, 68, 256, "inplace"), (70, 196, 768, "residual")], ids=lambda v: str(v))
def test_gemm_strides(m, n, k, epilogue, bf16):
    """lda = k + 4 (NaN padding) and ldy = n + 4 (sentinel padding): one unsplit shape, two split ones."""
    _gemm(f"prefill_gemm {WIDS[bf16]} {m}x{n}x{k} strided", 3000 + m + n + k, m, n, k, bf16, epilogue=epilogue, pad_a=4, pad_y=4)


@pytest.mark.parametrize("bf16", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("m,n,k", [(65, 68, 256), (33, 64, 512), (65, 132, 1280)], ids=lambda v: str(v))
def test_gemm_split_against_unsplit(m, n, k, bf16):
    """The same inputs with and without the scratch: the same sum in another order, so within the bar of each other, not bit-equal
    by right."""
    name = f"prefill_gemm {WIDS[bf16]} {m}x{n}x{k}"
    ys, used = _gemm(name, 4000 + m + n + k, m, n, k, bf16, split=True, epilogue="bias")
    yu, one = _gemm(name + " unsplit", 4000 + m + n + k, m, n, k, bf16, split=False, epilogue="bias")
    assert used > 1 and one == 1
    bar = TOL * max(1.0, float(np.abs(yu).max()))
    assert report(name + " split - unsplit", np.abs(ys.astype(np.float64) - yu).max(), bar) < bar


@pytest.mark.parametrize("bf16", WEIGHTS, ids=WIDS)
@pytest.mark.parametrize("m,n,k,grid", [(24, 64, 32, 1), (33, 64, 512, 4), (100, 132, 320, 12), (65, 132, 1280, 48), (65, 16448, 256, 514),
                                        (65, 4160, 1024, 520)], ids=lambda v: str(v))
def test_gemm_tile_order_covers_every_element_once(m, n, k, grid, bf16):
    """The XCD-aware remap of blockIdx must be a bijection at every grid size (grid % 8 = 1, 4, 4, 0, 2, 0 here).  One-hot rows of A
    pick column i of W for row i, and W holds integers, so every Y[i, j] is exact: a tile computed twice and another not at all
    shows as the sentinel, a slice added twice or dropped as a wrong integer.  f32 weights: 1 + j * k + c, distinct over the whole
    matrix; bf16 weights hold 8 significant bits, so the integers there are 1 .. 255 (a pattern of period 255 in 7 j + 3 c)."""
    assert P.geometry(m, n, k)[1] == grid and m <= k
    a = np.full((m + 3, k), np.nan, np.float32)
    a[:m] = 0.0
    a[np.arange(m), np.arange(m)] = 1.0
    j, c = np.arange(n, dtype=np.int64)[:, None], np.arange(k, dtype=np.int64)[None, :]
    wi = ((7 * j + 3 * c) % 255 + 1) if bf16 else (1 + j * k + c)
    assert wi.max() < (256 if bf16 else 1 << 24)
    w = wi.astype(np.float32)
    if bf16:
        w16 = ops.to_bf16(w)
        assert np.array_equal(ops.bf16_to_f32(w16), w)
        w = w16
    y = np.full((m, n), SENTINEL, np.float32)
    got, _, used = ops.prefill_gemm(a, w, m, y, bf16=bf16)
    assert used == P.ksplit_rule(m, n, k)
    want = wi[:, :m].T.astype(np.float32)
    assert not (got == SENTINEL).any(), f"{int((got == SENTINEL).sum())} elements were never written"
    assert np.array_equal(got, want), f"{int((got != want).sum())} elements hold a wrong integer"


# ---- the attention --------------------------------------------------------------------------------------------------------------------

def _att_inputs(rng, rows, base, heads, d, kv_group, pads=(0, 0, 0, 0)):
    """q, flat K, flat V, ldk, ldv, ctx: standard normal where the kernel may read, NaN in q's, K's and V's padding columns and in
    the three K / V rows behind the last key, the sentinel all over ctx."""
    pq, pk, pv, pc = pads
    kvd, n = heads // kv_group * d, base + rows
    q = np.full((rows, heads * d + pq), np.nan, np.float32)
    q[:, :heads * d] = rng.standard_normal((rows, heads * d)).astype(np.float32)
    k = np.full((n + 3, kvd + pk), np.nan, np.float32)
    v = np.full((n + 3, kvd + pv), np.nan, np.float32)
    k[:n, :kvd] = rng.standard_normal((n, kvd)).astype(np.float32)
    v[:n, :kvd] = rng.standard_normal((n, kvd)).astype(np.float32)
    ctx = np.full((rows, heads * d + pc), SENTINEL, np.float32)
    return q, k, v, ctx


def _check_ctx(name, got, ref, width, tol=TOL):
    assert np.array_equal(_bits(got[:, width:]), _bits(np.full_like(got[:, width:], SENTINEL))), "the padding columns of ctx were written"
    got = got[:, :width]
    assert got.shape == ref.shape
    assert np.isfinite(got).all(), "the context holds NaN / inf: a row behind the last key or a padding column was used"
    err = report(name, np.abs(got - ref).max(), tol)
    print(f"{name}: max |kernel - float64| = {err:.3e} (bar {tol:.1e})")
    assert err < tol, err


def _attention(name, seed, rows, base, heads, d, kv_group, route, pads=(0, 0, 0, 0)):
    rng = np.random.default_rng(seed)
    q, k, v, ctx = _att_inputs(rng, rows, base, heads, d, kv_group, pads)
    got, took = ops.prefill_attention(q, k, v, k.shape[1], v.shape[1], base, heads, d, kv_group=kv_group, ctx=ctx)
    assert took == route, (took, route)
    ref = R.attention64(q, k, v, k.shape[1], v.shape[1], base + rows, heads, d, causal_base=base, kv_group=kv_group)
    _check_ctx(name, got, ref, heads * d)
    return q, k, v, ref


def _edge_cases(all_rows, all_bases, full_rows, full_base, extra):
    cases = [(full_rows, b) for b in all_bases] + [(r, full_base) for r in all_rows if r != full_rows] + list(extra)
    assert len(set(cases)) == len(cases)
    return cases


# rows % 32 in {1, 31, 0}, several query blocks; base % 64 in {0, 1, 63}, cached keys in 0 .. 4 tiles
VEC_ROWS, VEC_BASES = [1, 31, 32, 33, 70], [0, 1, 63, 64, 65, 200]
VEC_EDGES = _edge_cases(VEC_ROWS, VEC_BASES, 33, 63, [(1, 0), (32, 0), (70, 0), (31, 1), (70, 64), (32, 65), (31, 200), (70, 200)])
VEC_CASES = [(d, r, b) for d in (32, 128) for r, b in VEC_EDGES] + [(d, r, b) for d in (16, 64) for r, b in ((33, 65), (70, 63))]


@pytest.mark.parametrize("d,rows,base", VEC_CASES)
def test_vector_kernel_block_and_tile_edges(d, rows, base):
    """prefill_attention_kernel<DPT> at every head width: the `limit` test and the `last_key` clamp at every rows % 32 and
    base % 64 edge (all bases at rows = 33, all row counts at base = 63, for widths 32 and 128)."""
    _attention(f"prefill_attention vector d={d} rows={rows} base={base}", 5000 + d + 7 * rows + base, rows, base, 2, d, 1, 0)


@pytest.mark.parametrize("pads", [(4, 8, 4, 8), (8, 4, 8, 4)], ids=str)
@pytest.mark.parametrize("kv_group,heads", [(1, 3), (2, 4), (7, 14)])
def test_vector_kernel_grouped_heads_and_strides(kv_group, heads, pads):
    _attention(f"prefill_attention vector gqa {kv_group}x{heads} pads {pads}", 5500 + heads, 33, 65, heads, 32, kv_group, 0, pads)


@pytest.mark.parametrize("d,rows,base", [(16, 300, 129), (32, 300, 129), (64, 255, 1), (128, 255, 64)])
def test_vector_kernel_long_blocks(d, rows, base):
    """Widths 16 and 32 stay on the vector kernel at any length; 64 and 128 up to 255 rows, the last length before the switch."""
    _attention(f"prefill_attention vector d={d} rows={rows} base={base}", 5600 + d, rows, base, 2, d, 1, 0)


# rows % 32 and % 128 in {0, 1}, two to four query blocks; base % 128 in {0, 1, 126, 127}.  base = 126 is the one value at which a
# chunk's last key is one past what a wave's first query sees (key0 + 127 == base + q_wave0 + 1): the `plain` test from its far side.
MFMA_ROWS, MFMA_BASES = [256, 257, 288, 289, 385], [0, 1, 127, 128, 129, 301]
MFMA_EDGES = _edge_cases(MFMA_ROWS, MFMA_BASES, 257, 127, [(257, 126), (256, 0), (385, 301), (288, 128), (289, 1)])
MFMA_CASES = ([(64, r, b, 3, 1, (0, 0, 0, 0)) for r, b in MFMA_EDGES] +
              [(128, r, b, 2, 2, (4, 8, 4, 8)) for r, b in ((257, 0), (257, 126), (257, 127), (257, 128), (256, 127), (385, 129), (289, 301))] +
              [(64, 256, 1, 1, 1, (8, 4, 8, 4)), (128, 288, 1, 3, 1, (0, 0, 0, 0)), (64, 289, 129, 2, 2, (4, 4, 4, 4))])


@pytest.mark.parametrize("d,rows,base,heads,kv_group,pads", MFMA_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_matrix_core_kernel_diagonal_edges(d, rows, base, heads, kv_group, pads):
    """prefill_attention_mfma_kernel<D>: `plain`, the chunk skip and n_chunks at every base % 128 edge (all bases at rows = 257) and
    every rows % 32 / % 128 edge (all row counts at base = 127); one, two and three heads (an odd count; the upper half walks the
    query blocks in reverse), grouped heads, padded strides."""
    _attention(f"prefill_attention mfma d={d} rows={rows} base={base} heads={heads}/{kv_group}", 6000 + d + 7 * rows + base, rows, base, heads, d,
               kv_group, 1, pads)


def _mask_probe(name, seed, rows, base, d, route, probes):
    """The mask matters, and it sits exactly on the diagonal: with key base + s + 1 (K and V) moved to other finite values the rows
    up to s keep their bits and row s + 1, whose last visible key it is, changes in every head."""
    heads = 2
    q, k, v, ref = _attention(name, seed, rows, base, heads, d, 1, route)
    n = base + rows
    unmasked = R.attention64(q[:8], k, v, k.shape[1], v.shape[1], n, heads, d)
    assert np.abs(unmasked - ref[:8]).max() > 1e-2, "without the mask the reference is the same: the case would not notice"
    ctx = np.full((rows, heads * d), SENTINEL, np.float32)
    first, _ = ops.prefill_attention(q, k, v, k.shape[1], v.shape[1], base, heads, d, ctx=ctx)
    for s in probes:
        assert -1 <= s < rows - 1
        k2, v2 = k.copy(), v.copy()
        k2[base + s + 1, :heads * d] = k[base + s + 1, :heads * d] * np.float32(-0.5) + np.float32(1.5)
        v2[base + s + 1, :heads * d] = v[base + s + 1, :heads * d] + np.float32(3.0)
        got, took = ops.prefill_attention(q, k2, v2, k.shape[1], v.shape[1], base, heads, d, ctx=ctx)
        assert took == route
        assert np.array_equal(_bits(got[:s + 1]), _bits(first[:s + 1])), f"key {base + s + 1} is invisible to rows 0 .. {s}, yet they changed"
        for h in range(heads):
            assert np.abs(got[s + 1, h * d:(h + 1) * d] - first[s + 1, h * d:(h + 1) * d]).max() > 1e-4, \
                f"key {base + s + 1} is row {s + 1}'s last visible key, yet head {h} of that row did not change"


def test_vector_kernel_mask_sits_on_the_diagonal():
    # keys 64 and 128 open a tile (s = 0, 64), 63 and 127 close one; rows 31 | 32 and 63 | 64 are query-block edges
    _mask_probe("prefill_attention vector mask", 7000, 70, 63, 32, 0, [-1, 0, 1, 30, 31, 32, 62, 63, 64, 68])


def test_matrix_core_kernel_mask_sits_on_the_diagonal():
    # keys 128, 256, 384 open a chunk (s = 0, 128, 256); rows 31 | 32 are wave edges, 127 | 128 and 255 | 256 workgroup edges
    _mask_probe("prefill_attention mfma mask", 7100, 289, 127, 64, 1, [-1, 0, 1, 30, 31, 32, 126, 127, 128, 129, 255, 256, 287])


# ---- scores far from zero ----------------------------------------------------------------------------------------------------------------

def _stress(name, seed, d, rows, base, levels, route, tol=TOL):
    """Scores exact in float32 (asserted), at the levels given per key -- the same for every query row."""
    rng = np.random.default_rng(seed)
    n = base + rows
    assert len(levels) == n
    q, kk = R.exact_score_inputs(rng, d, levels, rows=rows, heads=2)
    scale = 1.0 / np.sqrt(float(d))
    sc32 = (q.reshape(rows, 2, d).transpose(1, 0, 2) @ kk.reshape(n, 2, d).transpose(1, 2, 0)) * np.float32(scale)
    sc64 = (q.astype(np.float64).reshape(rows, 2, d).transpose(1, 0, 2) @ kk.astype(np.float64).reshape(n, 2, d).transpose(1, 2, 0)) * scale
    assert sc32.dtype == np.float32 and np.array_equal(sc32.astype(np.float64), sc64), "the scores are not exact in float32"
    assert np.abs(sc64).max() <= 72.0
    k = np.full((n + 3, 2 * d), np.nan, np.float32)
    v = np.full((n + 3, 2 * d), np.nan, np.float32)
    k[:n] = kk
    v[:n] = rng.standard_normal((n, 2 * d)).astype(np.float32)
    ctx = np.full((rows, 2 * d), SENTINEL, np.float32)
    got, took = ops.prefill_attention(q, k, v, 2 * d, 2 * d, base, 2, d, ctx=ctx)
    assert took == route
    ref = R.attention64(q, k, v, 2 * d, 2 * d, n, 2, d, causal_base=base)
    _check_ctx(name, got, ref, 2 * d, tol)
    return ref, v, sc64


# (kernel, d, rows, base, key tile): three key tiles each
STRESS = [("vector", 16, 70, 60, 64, 0), ("vector", 64, 70, 60, 64, 0), ("mfma", 64, 257, 127, 128, 1)]
STRESS_IDS = [f"{s[0]}-d{s[1]}" for s in STRESS]


@pytest.mark.parametrize("where", ["first-tile", "last-tile", "diagonal"])
@pytest.mark.parametrize("kernel,d,rows,base,tile,route", STRESS, ids=STRESS_IDS)
def test_one_key_far_above_the_rest(kernel, d, rows, base, tile, route, where):
    """One key 40 above the rest: every row that sees it is that key's V row to within exp(-30), the others are not.  In the first
    tile every later tile's weight is exp(-40) next to the running maximum; in the last tile, or on a row's diagonal, the running
    sums are scaled down by exp(-40) when it arrives."""
    n = base + rows
    at = {"first-tile": 2, "last-tile": n - 2, "diagonal": base + rows // 2}[where]
    assert (n - 1) // tile == 2 and (where != "first-tile" or at // tile == 0) and (where != "last-tile" or at // tile == 2)
    levels = np.zeros(n)
    levels[at] = 40.0
    ref, v, sc = _stress(f"prefill_attention {kernel} d={d} peak {where}", 8000 + d + at, d, rows, base, levels, route)
    assert (sc[:, :, at] - np.delete(sc, at, axis=2).max(axis=2) > 30).all()
    sees = np.arange(rows) + base >= at
    assert sees.any() and (where == "first-tile" or not sees.all())
    assert np.abs(ref[sees] - v[at].astype(np.float64)).max() < 1e-8


@pytest.mark.parametrize("low", [0, 1])
@pytest.mark.parametrize("kernel,d,rows,base,tile,route", STRESS, ids=STRESS_IDS)
def test_a_tile_whose_weight_underflows(kernel, d, rows, base, tile, route, low):
    """A whole key tile at -60 next to tiles at +55: exp(-115) is 0 in float32.  As the first tile it is everything the early rows
    see, and the rows behind it drop it with alpha = 0 when the next tile arrives; as the middle tile its probabilities are all 0
    under the running maximum."""
    n = base + rows
    levels = np.full(n, 55.0)
    levels[low * tile:(low + 1) * tile] = -60.0
    _, _, sc = _stress(f"prefill_attention {kernel} d={d} underflowing tile {low}", 8100 + d + low, d, rows, base, levels, route)
    assert (sc.max(axis=2) - sc[:, :, low * tile:(low + 1) * tile].max(axis=2) > 110).all()
    if low == 0:
        assert base < tile, "no row sees the low tile alone"


@pytest.mark.parametrize("level", [60.0, -60.0])
@pytest.mark.parametrize("kernel,d,rows,base,tile,route", STRESS, ids=STRESS_IDS)
def test_every_score_far_from_zero(kernel, d, rows, base, tile, route, level):
    """All scores near +60, or near -60: only the subtraction of the maximum keeps the exponentials in range and precise."""
    levels = np.full(base + rows, level)
    _, _, sc = _stress(f"prefill_attention {kernel} d={d} level {level:+.0f}", 8200 + d + int(level), d, rows, base, levels, route)
    assert (np.abs(sc - level) < 12).all()
