"""The encoder's packed-row kernels alone, launcher by launcher (kjarni_hip_op_mask_lengths, _pack_index, _encoder_embed,
_encoder_rope, _attention_packed, _pool_packed, _small_linear, _row_softmax: one launcher call each on host arrays) against the
plain numpy references of tests/encoder_rows_ref64.py.

Bars: 1e-5 absolute for attention on standard-normal inputs, LayerNorm, pooling and probabilities; 1e-5 * max(1, max|ref|) for the
head GEMV (test_gpu_ops.py).  Bit for bit: lengths, indices, the embedding without LayerNorm, RoPE, the exact
probes.  Every attention case holds the reported route against the restated rule; every case runs twice for the same bits and
finds its NaN pattern in every element the kernel does not own (the hooks check the guard bands behind every device buffer)."""
import numpy as np
import pytest

from kjarni_amd import ops
from tests import encoder_rows_ref64 as R
from tests.parity_report import report

pytestmark = pytest.mark.gpu

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
PAT = U32(0x7FC0ABCD)                       # a NaN no kernel produces
LSET = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
WORST = {}


def pat(*shape, dtype=F32):
    return np.full(shape, PAT, U32).view(dtype)


def is_pat(a):
    return np.ascontiguousarray(a).view(U32) == PAT


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(U32), np.ascontiguousarray(b).view(U32))


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if isinstance(x, np.ndarray):
            assert same_bits(x, y), "two runs of the same call differ"
        else:
            assert x == y
    return a


def hold(group, case, got, ref, bar):
    err = float(np.abs(np.asarray(got, F64) - ref).max())
    assert err == err, f"{group} {case}: NaN"
    ratio = err / bar
    if ratio >= WORST.get(group, (0.0,))[0]:
        WORST[group] = (ratio, err, bar, case)
    print(f"[encoder_rows] {group} {case}: err {err:.3e} bar {bar:.3e} ({ratio:.2f} of it)")
    report(f"encoder_rows {group}: largest err / bar", ratio, 1.0)
    assert err <= bar, f"{group} {case}: err {err:.3e} > bar {bar:.3e}"


# ---- lengths and the pack index ------------------------------------------------------------------------------------------------------

def _plain_mask(B, S, seed):
    """Right padding and holes, token 0 always kept, values 0 / 1: a plan the encoder packs."""
    rng = np.random.default_rng(seed)
    m = np.zeros((B, S), U32)
    for b in range(B):
        n = int(rng.integers(1, S + 1))
        m[b, :n] = 1
        if b % 3 == 1 and S > 2:
            m[b, 1:] = rng.integers(0, 2, S - 1)            # holes
    if S >= 64:
        m[0, :] = 0
        m[0, [0, 63]] = 1                                    # a kept token in lane 63 of a ballot
        if S >= 128:
            m[0, 127] = 1
    m[-1, :] = 1
    return m


def _odd_mask(B, S, seed):
    """The rows mask_lengths must flag as well: token 0 masked, an all-masked row, values 2 and 0xFFFFFFFF."""
    m = _plain_mask(B, S, seed)
    for b in range(B):
        if b % 5 == 1:
            m[b, 0] = 0
        elif b % 5 == 2:
            m[b, :] = 0
        elif b % 5 == 3:
            m[b, S - 1] = 2
        elif b % 5 == 4:
            m[b, S // 2] = 0xFFFFFFFF
    return m


SHAPES = [(B, S) for B in (1, 3, 4, 5, 9) for S in (1, 63, 64, 65, 128, 129, 200, 512)] + [(1000, 1), (1000, 65), (1000, 200)]


@pytest.mark.parametrize("B,S", SHAPES)
def test_mask_lengths(B, S):
    for mask in (_plain_mask(B, S, B * 1000 + S), _odd_mask(B, S, B * 1000 + S)):
        want = R.mask_lengths(mask)
        got = twice(lambda: ops.mask_lengths(mask, np.full(B, PAT, U32)))
        assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[:8], want[:8])
    if B >= 5:
        assert (want[[1, 2, 3, 4]] >> 31).all() and want[2] == 0x80000000     # the flagged rows are flagged


@pytest.mark.parametrize("B,S", SHAPES)
def test_pack_index(B, S):
    mask = _plain_mask(B, S, B * 1000 + S)
    assert not (R.mask_lengths(mask) >> 31).any()                              # a plan the encoder would take
    cu, src = R.pack_index(mask)
    got = twice(lambda: ops.pack_index(mask, cu, pat(len(src) + 64, dtype=I32)))
    assert np.array_equal(got[:len(src)], src)
    assert is_pat(got[len(src):]).all(), "tok_src written behind the last kept token"


def test_pack_index_keeps_lane_63():
    mask = np.zeros((2, 130), U32)
    mask[0, [0, 63, 64, 127, 128]] = 1
    mask[1, [0, 62, 63, 129]] = 1
    cu, src = R.pack_index(mask)
    assert src.tolist() == [0, 63, 64, 127, 128, 130, 192, 193, 259]
    got = twice(lambda: ops.pack_index(mask, cu, pat(16, dtype=I32)))
    assert np.array_equal(got[:9], src) and is_pat(got[9:]).all()


# ---- embedding -----------------------------------------------------------------------------------------------------------------------

def _embed_tables(H, seed, V=11, P=5, T=3, B=3, S=6):
    rng = np.random.default_rng(seed)
    word, pos, typ = (rng.standard_normal((n, H)).astype(F32) for n in (V, P, T))
    ids = rng.integers(0, V, (B, S)).astype(U32)
    ids.reshape(-1)[[0, 3, 7, 11]] = [0, V - 1, V, 0xFFFFFFFF]
    tys = rng.integers(0, T, (B, S)).astype(U32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(H)).astype(F32), (0.1 * rng.standard_normal(H)).astype(F32)
    mask = np.ones((B, S), U32)
    mask[0, 4:] = 0
    mask[1, [1, 2, 5]] = 0                                                      # holes
    _, src = R.pack_index(mask)
    src = np.concatenate([src, [0, 3, 7, 11]]).astype(I32)                      # (the edge ids are in whatever the mask keeps)
    return word, pos, typ, ids, tys, gamma, beta, src


@pytest.mark.parametrize("H", [4, 384, 768, 1024, 6, 1028])
def test_embedding(H):
    V, P, T, B, S = 11, 5, 3, 3, 6
    word, pos, typ, ids, tys, gamma, beta, src = _embed_tables(H, H)
    i = 0
    for variant in ("all", "no_pos", "no_type", "no_type_ids"):
        for eps in (None, 1e-12, 1e-5):
            for packed in (False, True):
                off, scale = (0, 2)[i % 2], bool((i // 2) % 2)
                i += 1
                p = None if variant == "no_pos" else pos
                t = None if variant == "no_type" else typ
                ty = None if variant in ("no_type", "no_type_ids") else tys
                rows_src = src if packed else np.arange(B * S, dtype=I32)
                raw = R.embed_f32(ids, word, p, t, ty, S, V, P if p is not None else 0, T if t is not None else 0, off, scale, rows_src)
                got = twice(lambda: ops.encoder_embed(ids, word, pat(len(rows_src), H), pos=p, type=t, type_ids=ty, gamma=None if eps is None else gamma,
                                                      beta=None if eps is None else beta, eps=eps or 0.0, pos_offset=off, scale_embeddings=scale,
                                                      tok_src=rows_src if packed else None))
                case = f"H={H} {variant} eps={eps} packed={packed} off={off} scale={scale}"
                if eps is None:
                    assert same_bits(got, raw), case
                else:
                    hold("embed+LayerNorm", case, got, R.layer_norm(raw, gamma, beta, eps), 1e-5)


def test_embedding_positions_either_side_of_max_pos():
    H, V, S = 8, 4, 6
    rng = np.random.default_rng(3)
    word, pos = rng.standard_normal((V, H)).astype(F32), rng.standard_normal((8, H)).astype(F32)
    ids = np.ones((1, S), U32)
    for off, max_pos in ((0, 5), (0, 6), (2, 5), (2, 7), (2, 8), (0, 1)):
        got = twice(lambda: ops.encoder_embed(ids, word, pat(S, H), pos=pos, max_pos=max_pos, pos_offset=off))
        for s in range(S):
            want = word[1] + pos[off + s] if off + s < max_pos else word[1]
            assert same_bits(got[s], want.astype(F32)), (off, max_pos, s)


@pytest.mark.parametrize("rows", range(1, 69))
def test_embedding_deals_every_row_once(rows):
    """Grids of 1 .. 17 workgroups: xcd_contiguous must deal every row exactly once for every remainder mod 8."""
    H, V = 4, 80
    word = np.arange(V * H, dtype=F32).reshape(V, H)
    ids = ((np.arange(70) * 37 + rows) % V).astype(U32).reshape(1, 70)
    got = twice(lambda: ops.encoder_embed(ids, word, pat(rows, H)))
    assert same_bits(got, word[ids[0, :rows]])
    src = ((np.arange(rows) * 13 + 5) % 70).astype(I32)
    got = twice(lambda: ops.encoder_embed(ids, word, pat(rows, H), tok_src=src))
    assert same_bits(got, word[ids[0, src]])


# ---- RoPE ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [2, 6, 8, 32, 64])
@pytest.mark.parametrize("heads", [1, 3, 12])
def test_rope(d, heads):
    S, B = 7, 3
    rng = np.random.default_rng(d * 100 + heads)
    cos, sin = (rng.uniform(-1, 1, (S, d)).astype(F32) for _ in range(2))
    mask = np.ones((B, S), U32)
    mask[0, 3:] = 0
    mask[1, [2, 4]] = 0
    _, src = R.pack_index(mask)
    for tok_src, positions in ((None, np.arange(B * S) % S), (src, src % S)):
        qkv = rng.standard_normal((len(positions), 3 * heads * d)).astype(F32)
        want = R.rope_f32(qkv, cos, sin, heads, d, positions)
        got = twice(lambda: ops.encoder_rope(qkv, cos, sin, heads, d, tok_src=tok_src))
        assert same_bits(got[:, 2 * heads * d:], qkv[:, 2 * heads * d:]), "the V third changed"
        assert same_bits(got, want), np.argwhere(got.view(U32) != want.view(U32))[:4]
    assert len(set((src % S).tolist())) > 1 and not np.array_equal(src % S, np.arange(len(src)) % S)   # packed positions differ from row % S


def test_rope_grid_stride_loop_runs_twice():
    """The scalar form at head_dim 6: 30 000 rows x 2 x 12 x 3 pairs = 2 160 000 > 256 x 32 x 256 threads."""
    d, heads, rows, S = 6, 12, 30000, 512
    assert rows * 2 * heads * (d // 2) > 256 * 32 * 256
    rng = np.random.default_rng(9)
    cos, sin = (rng.uniform(-1, 1, (S, d)).astype(F32) for _ in range(2))
    qkv = rng.standard_normal((rows, 3 * heads * d)).astype(F32)
    src = rng.integers(0, 64 * S, rows).astype(I32)
    got = twice(lambda: ops.encoder_rope(qkv, cos, sin, heads, d, tok_src=src))
    assert same_bits(got, R.rope_f32(qkv, cos, sin, heads, d, src % S))


# ---- attention on cu -----------------------------------------------------------------------------------------------------------------

def _lengths(n, seed, cap=128, must=()):
    """n lengths: `must`, then LSET in turn, then random ones up to cap."""
    rng = np.random.default_rng(seed)
    out = list(must) + [v for v in LSET if v <= cap]
    while len(out) < n:
        out.append(int(rng.integers(1, cap + 1)))
    return out[:n]


def run_attention(case, lengths, heads, d, seed=0, max_len=None, want_kernel=None, qkv=None, tail=0, nan_sentences=(), nan_tail=False, compare=True,
                  mask_value=-1e9):
    """One call (twice): the route against the rule, the tail rows of ctx untouched, every sentence outside `nan_sentences` against
    float64.  Returns (qkv, ctx)."""
    rows, H, B = int(np.sum(lengths)), heads * d, len(lengths)
    cu = R.cu_of(lengths)
    if qkv is None:
        qkv = np.random.default_rng(seed).standard_normal((rows + tail, 3 * H)).astype(F32)
    qkv = qkv.copy()
    for b in nan_sentences:
        qkv[cu[b]:cu[b + 1]] = np.nan
    if nan_tail:
        qkv[rows:] = np.nan
    ml = max(lengths) if max_len is None else max_len
    ctx, route = twice(lambda: ops.attention_packed(qkv, lengths, heads, d, pat(rows + tail, H), max_len=ml, mask_value=mask_value))
    assert route == R.attention_route(B, ml, heads, d, H % 4 == 0, True), (route, case)
    if want_kernel is not None:
        assert route[0] == want_kernel, (route, case)
    assert is_pat(ctx[rows:]).all(), f"{case}: ctx rows behind the last sentence were written"
    if compare:
        safe = np.nan_to_num(qkv.astype(F64))
        ref = R.attention_packed(safe[:rows], lengths, heads, d)
        keep = np.ones(rows, bool)
        for b in nan_sentences:
            keep[cu[b]:cu[b + 1]] = False
        assert not is_pat(ctx[:rows][keep]).any(), f"{case}: a context row was not written"
        hold(f"attention {('nothing', 'split', 'pipe0', 'pipe', 'pipe2', 'chunked', 'generic')[route[0]]}", f"{case} d={d}", ctx[:rows][keep], ref[keep], 1e-5)
    return qkv, ctx


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("B,heads", [(1, 12), (2, 12), (10, 12), (32, 4)])
def test_attention_small_call_kernel(B, heads, d):
    sets = {1: ([128], [33], [1], [97]), 2: ([1, 128], [97, 31], [64, 65]), 10: (LSET[:10], LSET[3:]), 32: (_lengths(32, d), _lengths(32, d + 1)[::-1])}[B]
    for k, lengths in enumerate(sets):
        assert len(lengths) == B
        run_attention(f"split B={B} heads={heads} #{k}", lengths, heads, d, seed=B + k, want_kernel=R.SPLIT)
    # max_len larger than the longest sentence: the extra query blocks return early
    run_attention(f"split B={B} sized for 128, longest 40", ([40, 7, 33, 1] + [5, 32, 2] * 10)[:B], heads, d, seed=B, max_len=128, want_kernel=R.SPLIT)


@pytest.mark.parametrize("d,B,heads,grid", [(32, 33, 4, 132), (64, 33, 4, 132), (32, 156, 5, 768), (32, 111, 7, 768), (64, 172, 3, 512)])
def test_attention_pipe_kernel(d, B, heads, grid):
    """132 items on 132 workgroups (the xcd_contiguous start); more items than resident workgroups with a head count that does not
    divide the grid, and enough of them that a workgroup's second item lies past the last head of its sentence step: advance()
    wraps the head index."""
    lengths = _lengths(B, B * heads)
    assert set(LSET) <= set(lengths)
    items = B * heads
    assert items == grid or any(j % heads + grid % heads >= heads for j in range(items - grid)), "no workgroup wraps its head index"
    _, _ = run_attention(f"pipe B={B} heads={heads}", lengths, heads, d, seed=B, want_kernel=R.PIPE_PACKED)
    assert R.attention_route(B, 128, heads, d, True, True)[1] == grid


@pytest.mark.parametrize("d", [32, 64])
def test_attention_pipe_kernel_whole_tiles_and_single_tokens(d):
    run_attention("pipe multiples of 32 (no_mask)", [32, 64, 96, 128] * 9, 4, d, seed=1, want_kernel=R.PIPE_PACKED)
    run_attention("pipe length 1 only", [1] * 40, 4, d, seed=2, want_kernel=R.PIPE_PACKED)
    run_attention("pipe length 1 only, sized for 128", [1] * 40, 4, d, seed=2, max_len=128, want_kernel=R.PIPE_PACKED)


@pytest.mark.parametrize("d", [32, 64])
def test_attention_chunked_kernel(d):
    run_attention("chunked", [129, 1, 128, 200, 256, 257, 384, 5], 3, d, seed=4, want_kernel=R.CHUNKED)
    run_attention("chunked sized for 512", [129, 33, 1], 2, d, seed=5, max_len=512, want_kernel=R.CHUNKED)


@pytest.mark.parametrize("d", [8, 16, 48])
def test_attention_generic_kernel(d):
    run_attention("generic", [1, 2, 33, 64, 65, 128, 130, 7], 3, d, seed=6, want_kernel=R.GENERIC)


@pytest.mark.parametrize("kernel,d,heads,lengths", [(R.SPLIT, 32, 4, [1, 33, 128, 40]), (R.SPLIT, 64, 4, [97, 2]), (R.PIPE_PACKED, 64, 12, _lengths(13, 2)),
                                                    (R.CHUNKED, 32, 3, [129, 5, 200]), (R.GENERIC, 16, 2, [3, 70])])
def test_attention_on_cu_ignores_the_mask_value(kernel, d, heads, lengths):
    """Every packed row is a kept token: whatever a masked key would score must not reach the result."""
    qkv, want = run_attention("mask value -1e9", lengths, heads, d, seed=17, want_kernel=kernel)
    for mv in (0.0, 1e9, float("-inf")):
        _, got = run_attention(f"mask value {mv}", lengths, heads, d, qkv=qkv, want_kernel=kernel, mask_value=mv, compare=False)
        assert same_bits(got, want), f"mask_value {mv} changed a context row"


NEIGHBOUR_ROUTES = [("split", R.SPLIT, 32, 12, []), ("split", R.SPLIT, 64, 12, []), ("pipe", R.PIPE_PACKED, 32, 12, [17, 64, 128, 90, 5, 31]),
                    ("pipe", R.PIPE_PACKED, 64, 12, [17, 64, 128, 90, 5, 31]), ("pipe wrapped", R.PIPE_PACKED, 32, 5, None),
                    ("chunked", R.CHUNKED, 32, 3, [200]), ("chunked", R.CHUNKED, 64, 3, [200]), ("generic", R.GENERIC, 16, 3, [])]


@pytest.mark.parametrize("name,kernel,d,heads,fill", NEIGHBOUR_ROUTES)
def test_attention_neighbours(name, kernel, d, heads, fill):
    """A full 128-token sentence, one of 33 and one of a single token placed last (128 rows behind it in qkv) next to NaN: the
    sentence after each all NaN, then the sentence before each.  Their context rows are the clean run's bit for bit."""
    if fill is None:
        fill = _lengths(150, 11)                                               # 780 items on 768 workgroups
    lengths = fill + [40, 128, 50, 33, 60, 1]
    n = len(fill)
    targets = (n + 1, n + 3, n + 5)
    cu = R.cu_of(lengths)
    qkv, clean = run_attention(f"{name} neighbours clean", lengths, heads, d, seed=21, tail=128, want_kernel=kernel)
    for what, nans, tail_nan in (("after", (n + 2, n + 4), True), ("before", (n, n + 2, n + 4), False)):
        _, ctx = run_attention(f"{name} NaN {what}", lengths, heads, d, qkv=qkv, tail=128, nan_sentences=nans, nan_tail=tail_nan, want_kernel=kernel)
        for t in targets:
            rows = slice(int(cu[t]), int(cu[t + 1]))
            assert np.isfinite(ctx[rows]).all(), f"{name}: NaN {what} sentence {t - n} reached it"
            assert same_bits(ctx[rows], clean[rows]), f"{name}: NaN {what} sentence {t - n} changed it"


@pytest.mark.parametrize("name,kernel,d,heads,lengths", [
    ("split", R.SPLIT, 32, 4, [128, 1, 33, 64, 97, 5]), ("pipe", R.PIPE_PACKED, 32, 12, _lengths(20, 3)), ("pipe", R.PIPE_PACKED, 64, 12, _lengths(20, 4)),
    ("pipe capped", R.PIPE_PACKED, 32, 5, _lengths(156, 5)), ("chunked", R.CHUNKED, 64, 3, [129, 1, 128, 200, 257, 5]), ("generic", R.GENERIC, 48, 2, [1, 33, 130, 64])])
def test_attention_order_of_sentences(name, kernel, d, heads, lengths):
    """The same sentences packed in two orders (same item count, same route): every sentence's context rows bit for bit."""
    rng = np.random.default_rng(31)
    H = heads * d
    sent = [rng.standard_normal((n, 3 * H)).astype(F32) for n in lengths]
    perm = rng.permutation(len(lengths))
    assert not np.array_equal(perm, np.arange(len(lengths)))
    _, a = run_attention(f"{name} order a", lengths, heads, d, qkv=np.concatenate(sent), want_kernel=kernel)
    _, b = run_attention(f"{name} order b", [lengths[i] for i in perm], heads, d, qkv=np.concatenate([sent[i] for i in perm]), want_kernel=kernel, compare=False)
    cu_a, cu_b = R.cu_of(lengths), R.cu_of([lengths[i] for i in perm])
    for j, i in enumerate(perm):
        assert same_bits(a[cu_a[i]:cu_a[i + 1]], b[cu_b[j]:cu_b[j + 1]]), f"{name}: sentence {i} differs when packed at {j}"


@pytest.mark.parametrize("name,kernel,d,heads,reps,extra", [
    ("split", R.SPLIT, 32, 12, 1, []), ("split", R.SPLIT, 64, 12, 1, []), ("pipe", R.PIPE_PACKED, 32, 12, 2, []), ("pipe", R.PIPE_PACKED, 64, 12, 2, []),
    ("chunked", R.CHUNKED, 32, 3, 1, [256]), ("chunked", R.CHUNKED, 64, 3, 1, [256]), ("generic", R.GENERIC, 16, 3, 1, [256])])
def test_attention_exact_probes(name, kernel, d, heads, reps, extra):
    """Q = 0: every score is exactly 0 and every probability exactly 1 / len (len a power of two); with V small integers the context
    row is the exact mean of the sentence's V rows.  A key too many or too few changes it (checked on the data itself)."""
    lengths = ([1, 2, 4, 8, 16, 32, 64, 128] + extra) * reps
    rng = np.random.default_rng(41)
    rows, H = sum(lengths), heads * d
    qkv = np.zeros((rows + 1, 3 * H), F32)
    qkv[:, H:2 * H] = rng.standard_normal((rows + 1, H))
    qkv[:, 2 * H:] = rng.integers(-8, 9, (rows + 1, H))
    cu = R.cu_of(lengths)
    _, ctx = run_attention(f"{name} probes", lengths, heads, d, qkv=qkv, tail=1, want_kernel=kernel, compare=False)
    v = qkv[:, 2 * H:].astype(F64)
    for b, n in enumerate(lengths):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        mean = v[r0:r1].mean(axis=0)
        assert np.array_equal(mean.astype(F32).astype(F64), mean)              # the mean is an f32
        for h in range(heads):                                                 # one key more or fewer moves every head's mean
            cols = slice(h * d, (h + 1) * d)
            assert (v[r0:r1 + 1].mean(axis=0)[cols] != mean[cols]).any() and (n == 1 or (v[r0:r1 - 1].mean(axis=0)[cols] != mean[cols]).any())
            assert r0 == 0 or (v[r0 - 1:r1].mean(axis=0)[cols] != mean[cols]).any()
        want = np.broadcast_to(mean.astype(F32), (n, H))
        assert same_bits(ctx[r0:r1] + F32(0), want + F32(0)), f"{name}: sentence {b} of {n} tokens is not the exact mean of its V rows"


# ---- pooling -------------------------------------------------------------------------------------------------------------------------

def run_pool(case, hs, lengths, seq=None):
    cu = R.cu_of(lengths)
    for mode in (R.POOL_MEAN, R.POOL_CLS, R.POOL_MAX, R.POOL_LAST):
        for l2 in (False, True):
            got = twice(lambda: ops.pool_packed(hs, lengths, pat(len(lengths), hs.shape[1]), pooling=mode, normalize=l2, seq=seq))
            hold("pool", f"{case} mode={mode} l2={l2}", got, R.pool_packed(hs, lengths, mode, l2), 1e-5)
            if mode == R.POOL_CLS and not l2:
                assert same_bits(got, hs[cu[:-1]]), f"{case}: CLS is not the gathered first rows"
            if mode == R.POOL_LAST and not l2:
                assert same_bits(got, hs[cu[1:] - 1]), f"{case}: LAST is not the gathered last rows"


@pytest.mark.parametrize("H,lengths", [(384, [70, 71, 80, 81, 128, 512]), (768, [1, 2, 9, 17, 40]), (1024, [1, 2, 9, 17, 40]), (100, [1, 2, 39, 40, 41, 330]),
                                       (6, [1, 2, 9, 17, 40]), (1022, [1, 2, 9, 17, 40])])
def test_pool_on_cu_1024_threads(H, lengths):
    hs = np.random.default_rng(H).standard_normal((sum(lengths), H)).astype(F32)
    run_pool(f"wide H={H}", hs, lengths)
    run_pool(f"wide H={H} sized for 600", hs, lengths, seq=600)


def test_pool_on_cu_256_threads():
    """B = 2 048: two row groups at hidden 384, lengths 1 .. 20 either side of its eight-row unrolled loop (14 / 15 / 16 / 17)."""
    lengths = [1 + (b % 20) for b in range(2048)]
    hs = np.random.default_rng(7).standard_normal((sum(lengths), 384)).astype(F32)
    cu = R.cu_of(lengths)
    for mode, l2 in ((R.POOL_MEAN, True), (R.POOL_MEAN, False), (R.POOL_CLS, False), (R.POOL_MAX, False), (R.POOL_LAST, True)):
        got = twice(lambda: ops.pool_packed(hs, lengths, pat(2048, 384), pooling=mode, normalize=l2))
        hold("pool", f"256 threads mode={mode} l2={l2}", got, R.pool_packed(hs, lengths, mode, l2), 1e-5)
        if mode == R.POOL_CLS:
            assert same_bits(got, hs[cu[:-1]])
    hs6 = np.random.default_rng(8).standard_normal((sum(lengths), 6)).astype(F32)
    for mode in range(4):
        got = twice(lambda: ops.pool_packed(hs6, lengths, pat(2048, 6), pooling=mode, normalize=True))
        hold("pool", f"256 threads H=6 mode={mode}", got, R.pool_packed(hs6, lengths, mode, True), 1e-5)


def test_padded_pool_256_threads_with_a_mask():
    B, S, H = 2048, 20, 384
    rng = np.random.default_rng(10)
    hs = rng.standard_normal((B, S, H)).astype(F32)
    mask = np.zeros((B, S), U32)
    for b in range(B):
        mask[b, :1 + (b % S)] = 1
        if b % 7 == 3:
            mask[b, 1:] = rng.integers(0, 2, S - 1)
        if b % 97 == 5:
            mask[b, :] = 0                                                     # nothing kept: token 0
    for mode in range(4):
        for l2 in (False, True):
            got = twice(lambda: ops.pool(hs, mask, mode, l2))
            hold("pool", f"padded B=2048 mode={mode} l2={l2}", got, R.pool_padded(hs, mask, mode, l2), 1e-5)


def test_pool_zero_vector_under_l2():
    for H, B in ((384, 3), (6, 3), (384, 2048)):
        lengths = [3, 2, 4] + [1] * (B - 3)
        hs = np.random.default_rng(H).standard_normal((sum(lengths), H)).astype(F32)
        hs[3:5] = 0
        for mode in range(4):
            got = twice(lambda: ops.pool_packed(hs, lengths, pat(B, H), pooling=mode, normalize=True))
            assert same_bits(got[1] + F32(0), np.zeros(H, F32)), (H, B, mode)
            assert np.isfinite(got).all()


# ---- heads ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 100, 384, 1024])
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_small_linear(k, n):
    rng = np.random.default_rng(k * 10 + n)
    for rows, ld, with_bias in ((5, k, True), (5, k + 5, False), (1, k, False), (6, k + 384, True), (9, k, True)):
        feat = rng.standard_normal((rows, ld)).astype(F32)
        feat[:, k:] = np.nan                                                   # nothing past k of a row is read
        w, bias = rng.standard_normal((n, k)).astype(F32), rng.standard_normal(n).astype(F32) if with_bias else None
        ref = R.small_linear(feat, w, bias, k)
        got = twice(lambda: ops.small_linear(feat, w, bias, pat(rows, n), k=k))
        hold("small_linear", f"k={k} n={n} rows={rows} ld={ld} bias={with_bias}", got, ref, 1e-5 * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("rows", [1, 255, 256, 257])
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_row_softmax(rows, n):
    rng = np.random.default_rng(rows * 10 + n)
    x = (3 * rng.standard_normal((rows, n))).astype(F32)
    x[0] = 100.0
    x[0, ::2] = -100.0
    x[-1] = 1.25                                                               # equal logits
    if rows > 2:
        x[1] = -100.0
        x[1, -1] = 100.0
    for sigmoid in (False, True):
        got = twice(lambda: ops.row_softmax(x, pat(rows, n), sigmoid=sigmoid))
        hold("probabilities", f"rows={rows} n={n} sigmoid={sigmoid}", got, R.row_softmax(x, sigmoid), 1e-5)
        if not sigmoid and rows > 1 and n > 1:
            assert (got[0, ::2] == 0).all() and abs(float(got[0].sum()) - 1) < 1e-6    # logits of -100 next to 100, of 100 alone


def test_worst_cases_are_reported():
    """(runs last in the file: the largest err / bar of every group, for the log)"""
    for group, (ratio, err, bar, case) in sorted(WORST.items()):
        print(f"[encoder_rows] worst {group}: {ratio:.3f} of the bar (err {err:.3e}, bar {bar:.3e}) at {case}")
