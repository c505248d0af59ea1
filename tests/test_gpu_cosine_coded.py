"""Cosine search over the int8 plane (cosine_coded.hip) against float64 numpy and against kjarni_hip_cosine_search on the same
inputs: the plane's numbers, the bound at its worst, the search bit for bit, order, rows the rule cannot judge, the filter's
pass rate, and the index switch end to end."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _gauss(n, dim, seed=0):
    x = np.random.default_rng([n, dim, seed]).standard_normal((n, dim)).astype(np.float32)
    x.setflags(write=False)
    return x


def _both(q, c, k, mode):
    """(coded idx, coded scores, stats, plain idx, plain scores)"""
    import kjarni_amd
    st = []
    i1, s1 = kjarni_amd.cosine_search(q, c, k, mode=mode, codes=True, stats=st)
    i0, s0 = kjarni_amd.cosine_search(q, c, k, mode=mode)
    return i1, s1, st, i0, s0


def _same_bits(i1, s1, i0, s0):
    assert np.array_equal(i1, i0)
    assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32))


@pytest.mark.parametrize("dim", [64, 384, 1024])
def test_encode(dim):
    """Codes = rint(d / s) with s = max|d| / 127 (f32, bit for bit); ||d|| = the streaming scan's norm, bit for bit; e at least the
    float64 residual norm and within 1 + 2^-16 of it (the kernel multiplies its f32 root by 1 + 2^-17; the f32 sum of squares and
    the root are within 2^-18); a zero row, a row with one 1e30 element and a NaN row are marked as not covered."""
    from kjarni_amd import ops
    x = _gauss(32, dim).copy()
    x[3] = 0.0
    x[5, 7] = 1e30
    x[9, 1] = np.nan
    codes, meta = ops.cosine_encode(x)
    fin = np.array([r for r in range(32) if r not in (3, 5, 9)])
    s = (np.abs(x[fin]).max(axis=1) / np.float32(127.0)).astype(np.float32)
    assert np.array_equal(meta[fin, 0].view(np.uint32), s.view(np.uint32))
    assert np.array_equal(codes[fin], np.rint(x[fin] / s[:, None]).astype(np.int8))
    norms = np.sqrt(ops.cosine_scores(x[0], x, mode=2)[0])
    assert np.array_equal(meta[fin, 2].view(np.uint32), norms[fin].view(np.uint32))
    res = np.linalg.norm(x[fin].astype(np.float64) - s.astype(np.float64)[:, None] * codes[fin], axis=1)
    assert (meta[fin, 1] >= res).all() and (meta[fin, 1] <= res * (1 + 2.0 ** -16)).all()
    assert (meta[fin, 3] == 1).all() and (meta[[3, 5, 9], 3] == 0).all()
    assert (codes[3] == 0).all() and meta[3, 0] == 0 and codes[5, 7] == 127 and (np.delete(codes[5], 7) == 0).all()


def _half_step_rows(n, dim, scale, seed):
    """Every element (m + 0.5) s with m even (rint goes to m: a residual of +s / 2 everywhere), one element 127 s: the scale is s."""
    m = 2 * np.random.default_rng(seed).integers(0, 63, (n, dim))
    x = ((m + 0.5) * scale).astype(np.float32)
    x[:, 0] = 127 * scale
    return x


def test_bound_holds_at_its_worst():
    """Rows and queries half a step from their codes, all residuals and codes of one sign: the float64 |q.d - s_q s c_q.c| against
    the bound formed from the kernel's own plane numbers, (||q|| + e_q) e + e_q ||d||, for every pair -- never above it, and
    close to it (a bound that is not slack by construction).  The search over such rows equals the exact one."""
    from kjarni_amd import ops
    d, q = _half_step_rows(20000, 128, 2.0 ** -7, 1), _half_step_rows(2, 128, 2.0 ** -6, 2)
    cd, md = ops.cosine_encode(d[:512])
    cq, mq = ops.cosine_encode(q)
    md, mq = md.astype(np.float64), mq.astype(np.float64)
    approx = np.outer(mq[:, 0], md[:, 0]) * (cq.astype(np.int64) @ cd.astype(np.int64).T)
    err = np.abs(q.astype(np.float64) @ d[:512].astype(np.float64).T - approx)
    bound = np.outer(mq[:, 2] + mq[:, 1], md[:, 1]) + np.outer(mq[:, 1], md[:, 2])
    ratio = err / bound
    print("largest error / bound:", ratio.max())
    assert ratio.max() <= 1.0 and ratio.max() > 0.5
    i1, s1, st, i0, s0 = _both(q, d, 10, 0)
    _same_bits(i1, s1, i0, s0)


# n_docs 20 000 / 20 007 / 50 001: tail tiles of 0, 7 and 1 documents; every dim, query count (1, 16, 17, 64, 65: the 1 / 2 / 4 query
# blocks and a second launch), k and mode of the issue's grid appears; fallback: 2 where the int8 passes do not serve the shape
# (dim 64; k = 256, above an eighth of the sample's 156 units), else 0
@pytest.mark.parametrize("n,dim,nq,k,mode,fallback", [(20000, 64, 17, 10, 0, 2), (20007, 128, 1, 1, 1, 0), (20007, 128, 16, 10, 0, 0),
                                                       (50001, 384, 65, 10, 1, 0), (50001, 384, 1, 10, 0, 0), (20000, 1024, 17, 1, 0, 0),
                                                       (20007, 384, 64, 256, 1, 2), (50001, 1024, 1, 10, 1, 0), (20000, 128, 64, 1, 1, 0)])
def test_search(n, dim, nq, k, mode, fallback):
    c, q = _gauss(n, dim), _gauss(nq, dim, seed=1)
    i1, s1, st, i0, s0 = _both(q, c, k, mode)
    print("stats", st)
    assert st[3] == fallback and (fallback or (st[0] == nq * n and st[1] >= st[2] >= nq * k))
    ref = (q.astype(np.float64) @ c.astype(np.float64).T) / np.outer(np.linalg.norm(q.astype(np.float64), axis=1),
                                                                     np.linalg.norm(c.astype(np.float64), axis=1))
    order = np.argsort(-ref, axis=1, kind="stable")[:, :k + 1]
    top = np.take_along_axis(ref, order, axis=1)
    assert np.abs(s1 - top[:, :k]).max() < 1e-4
    if nq >= 2:
        _same_bits(i1, s1, i0, s0)
    else:
        assert np.abs(s1 - s0).max() <= 2e-6
        clear = (-np.diff(top, axis=1) > 4e-6)
        clear = clear[:, :k] & np.concatenate([np.ones((nq, 1), bool), clear[:, :k - 1]], axis=1)   # both neighbours apart
        assert np.array_equal(i1[clear], order[:, :k][clear]) and np.array_equal(i0[clear], order[:, :k][clear])


def test_order_and_clustered():
    """Duplicate rows come out by ascending index, a best document planted at index 0 and in the last partial tile is found; a
    clustered corpus (every pair passes the filter) is right whether its lists hold that or overflow, and the stats say which."""
    c, q = _gauss(20007, 128).copy(), _gauss(2, 128, seed=1)
    c[0], c[20006] = 2 * q[0], 3 * q[1]
    c[[100, 300, 200]] = q[0] + 0.3 * _gauss(1, 128, seed=2)
    i1, s1, st, i0, s0 = _both(q, c, 10, 0)
    _same_bits(i1, s1, i0, s0)
    assert st[3] == 0 and i1[0, :4].tolist() == [0, 100, 200, 300] and i1[1, 0] == 20006
    near = (_gauss(1, 128, seed=3) + 0.01 * _gauss(20007, 128, seed=4)).astype(np.float32)
    i1, s1, st, i0, s0 = _both(q, near, 10, 1)
    print("clustered stats", st)
    _same_bits(i1, s1, i0, s0)
    assert st[3] == 1 or st[1] > 0.9 * st[0]


@pytest.mark.parametrize("mode", [0, 1])
def test_unjudgeable_rows_and_queries(mode):
    """Zero, tiny-norm, NaN and Inf rows pass the filter and are decided exactly; a query of that kind hands the call to the
    existing search: the same answers as kjarni_hip_cosine_search, mode 1's zero-norm rule among them."""
    c = _gauss(20007, 128).copy()
    c[4], c[20001] = 0.0, 1e-7 * c[20001]
    c[17, 3], c[20005, 5] = np.nan, np.inf
    good = _gauss(3, 128, seed=1)
    i1, s1, st, i0, s0 = _both(good, c, 10, mode)
    assert st[3] == 0 and np.array_equal(i1, i0) and np.array_equal(s1, s0, equal_nan=True)
    for fill in (0.0, 1e-7, np.nan, np.inf):   # query 1: zero, norm 1e-6, a NaN element, an Inf element
        qs = good.copy()
        if fill in (0.0, 1e-7):
            qs[1] *= np.float32(fill)
        else:
            qs[1, 2] = fill
        i1, s1, st, i0, s0 = _both(qs, c, 10, mode)
        assert st[3] == 1 and np.array_equal(i1, i0) and np.array_equal(s1, s0, equal_nan=True)
        if mode == 1 and fill == 0.0:
            assert (i1[1] == -1).all()
        i1, s1, st, i0, s0 = _both(qs[1], c, 10, mode)   # the same query alone
        assert np.array_equal(i1, i0) and np.array_equal(s1, s0, equal_nan=True)


def _numpy_pass_ratio(q, c, k):
    """The filter restated in numpy, same sample plan (units of one 16-document tile, 390 of them, 8 tiles apart at 50 001)."""
    def enc(x):
        s = np.abs(x).max(axis=1) / 127.0
        code = np.rint(x / s[:, None])
        return code, s, np.linalg.norm(x - s[:, None] * code, axis=1), np.linalg.norm(x, axis=1)
    (cq, sq, eq, nq_), (cd, sd, ed, nd) = enc(q.astype(np.float64)), enc(c.astype(np.float64))
    hat = (sq[0] * sd * (cd @ cq[0])) / (nq_[0] * nd)
    eps = ((nq_[0] + eq[0]) * ed + eq[0] * nd) / (nq_[0] * nd) + 384 * 2.0 ** -24 + 2.0 ** -18
    tiles = (len(c) + 15) // 16
    units = min(4096, tiles // 8)
    stride = tiles // units
    low = np.full(tiles * 16, -np.inf)
    low[:len(c)] = hat - eps
    maxima = low.reshape(tiles, 16)[np.arange(units) * stride].max(axis=1)
    return float(np.mean(hat + eps >= np.sort(maxima)[-k]))


def test_the_filter_filters():
    """Gaussian rows, 50 001 x 384, k = 10: no fallback, and passed / judged below four times the numpy restatement's ratio (the
    margin is for where the sample falls, not for the kernel's arithmetic).  Measured on an MI355X: 303 of 50 001 pairs pass, a ratio
    of 0.00606 -- the restatement's own figure, pair for pair."""
    c, q = _gauss(50001, 384), _gauss(1, 384, seed=1)
    expect = _numpy_pass_ratio(q, c, 10)
    i1, s1, st, i0, s0 = _both(q, c, 10, 0)
    print("numpy ratio", expect, "kernel ratio", st[1] / st[0], "stats", st)
    assert st[3] == 0 and st[1] / st[0] <= 4 * expect and expect < 0.05


@pytest.mark.parametrize("dim", [64, 128])
def test_index_switch_end_to_end(dim, tmp_path):
    """An index of 20 000 documents searched with the switch off and on: the same hits (scores within the 2e-6 of the one-query
    pass), and the image grows by exactly the plane.  (dim 64: a plane, but a width the int8 passes leave to the stream scan.)"""
    from oracle import search_oracle as SO
    from kjarni_amd import lib
    from kjarni_amd.searcher import index_image_bytes, index_search, set_index_codes
    rows = _gauss(20000, dim)
    root = str(tmp_path / "idx")
    SO.write_index(root, dim, [("t", rows[i], {}) for i in range(len(rows))], max_docs_per_segment=7000)
    q = _gauss(1, dim, seed=1)[0]
    try:
        before = index_image_bytes()
        off = index_search(root, None, q, mode="semantic", top_k=10)
        plain = index_image_bytes() - before
        set_index_codes(True)
        on = index_search(root, None, q, mode="semantic", top_k=10)
        assert index_image_bytes() - before - plain == lib().kjarni_hip_cosine_codes_bytes(20000, dim)
    finally:
        set_index_codes(False)
    assert plain == 20000 * dim * 4
    assert [h["document_id"] for h in on] == [h["document_id"] for h in off]
    assert max(abs(a["score"] - b["score"]) for a, b in zip(on, off)) <= 2e-6
