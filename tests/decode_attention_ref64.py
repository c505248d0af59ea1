"""Float64 reference of the decode attention and of the projections that merge its slabs, in plain numpy.

The attention knows nothing of key ranges: per (row, head) the scores q.k / sqrt(d) of ALL keys are taken in float64, masked
scores are overwritten with -1e9 (apply_causal_mask, utils/masks.rs), one softmax runs over the whole row and multiplies V.
Grouped-query heads, lanes, ragged lanes and strides are plain indexing into the flat K / V buffers the kernel is given."""
import numpy as np

MASK_VALUE = -1e9


def bf16_to_f64(w16):
    """bf16 bit patterns (uint16) widened exactly."""
    return (np.ascontiguousarray(w16, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def keys_of_row(s, n_keys, lane_pos=None, lane_live=None):
    """How many keys query row s sees: n_keys, or with ragged lanes min(lane_pos[s] + 1, capacity), 0 for a dead lane."""
    if lane_pos is None:
        return int(n_keys)
    return min(int(lane_pos[s]) + 1, int(n_keys)) if int(lane_live[s]) else 0


def scores64(q, k, ldk, n_keys, heads, d, causal_base=-1, kv_group=1, k_lane_stride=0, lanes=0, lane_pos=None, lane_live=None, dtype=np.float64):
    """Per row a [heads, n_row] array of masked scores and the boolean mask (True = masked) that was applied.  dtype float32
    takes the products and sums in float32 (for the exact-score inputs: they must come out the same)."""
    q = np.asarray(q)
    kf = np.asarray(k).reshape(-1)
    out, masks = [], []
    for s in range(q.shape[0]):
        n = keys_of_row(s, n_keys, lane_pos, lane_live)
        sc = np.zeros((heads, n), dtype)
        for h in range(heads):
            col = (h // kv_group) * d
            qv = q[s, h * d:(h + 1) * d].astype(dtype)
            for t in range(n):
                at = s * k_lane_stride + t * ldk + col
                kv = kf[at:at + d].astype(dtype)
                acc = dtype(0)
                for c in range(d):
                    acc = dtype(acc + qv[c] * kv[c])
                sc[h, t] = acc * dtype(1.0 / np.sqrt(float(d)))
        mask = np.zeros((heads, n), bool)
        if causal_base >= 0 and not lanes:
            mask[:, np.arange(n) > causal_base + s] = True
        sc[mask] = MASK_VALUE
        out.append(sc)
        masks.append(mask)
    return out, masks


def attention64(q, k, v, ldk, ldv, n_keys, heads, d, causal_base=-1, kv_group=1, k_lane_stride=0, v_lane_stride=0, lanes=0, lane_pos=None,
                lane_live=None):
    """ctx [rows, heads * d] in float64.  A row without keys (a dead lane) is zero."""
    q64 = np.asarray(q, np.float64)
    kf, vf = np.asarray(k, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
    rows = q64.shape[0]
    ctx = np.zeros((rows, heads * d), np.float64)
    for s in range(rows):
        n = keys_of_row(s, n_keys, lane_pos, lane_live)
        if n == 0:
            continue
        t = np.arange(n)
        for h in range(heads):
            col = (h // kv_group) * d
            kk = kf[(s * k_lane_stride + t * ldk + col)[:, None] + np.arange(d)[None, :]]      # [n, d]
            vv = vf[(s * v_lane_stride + t * ldv + col)[:, None] + np.arange(d)[None, :]]
            sc = kk @ q64[s, h * d:(h + 1) * d] / np.sqrt(float(d))
            if causal_base >= 0 and not lanes:
                sc[t > causal_base + s] = MASK_VALUE
            p = np.exp(sc - sc.max())
            ctx[s, h * d:(h + 1) * d] = (p / p.sum()) @ vv
    return ctx


def merge64(slabs):
    """slabs [heads, splits, d + 4] = (max, sum of exp, 0, 0, sum of exp * V) per key range -> the context row [heads * d]:
    every range weighs exp(max_i - M); an empty range (max -inf) weighs 0; a head with nothing at all stays zero."""
    sl = np.asarray(slabs, np.float64)
    heads, _, width = sl.shape
    d = width - 4
    ctx = np.zeros(heads * d, np.float64)
    for h in range(heads):
        m = sl[h, :, 0]
        live = np.isfinite(m)
        if not live.any():
            continue
        w = np.where(live, np.exp(np.where(live, m, 0.0) - m[live].max()), 0.0)
        total = (sl[h, :, 1] * w).sum()
        acc = (sl[h, :, 4:] * w[:, None]).sum(axis=0)
        ctx[h * d:(h + 1) * d] = acc / total if total > 0 else acc
    return ctx


def merge_project64(slabs, w, bias, r, bf16=False):
    """y = merge64(slabs) . w^T + bias + r; w f32, or bf16 bit patterns widened exactly."""
    w64 = bf16_to_f64(w) if bf16 else np.asarray(w, np.float64)
    y = w64 @ merge64(slabs)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    return y + np.asarray(r, np.float64)


def exact_score_inputs(rng, d, levels, rows=1, heads=2):
    """q [rows, heads * d] and K [n, heads * d] whose every score is exact in float32: 1 / sqrt(d) is a power of two at
    d = 4, 16, 64, every entry is a multiple of 0.25, and q[:, 0] = sqrt(d) turns K's first column into the score's level:
    score(t) = levels[t] + (a sum of at most d - 1 products of quarters in [-1, 1]) / sqrt(d)."""
    n = len(levels)
    quarters = lambda shape: (rng.integers(-4, 5, shape) * 0.25).astype(np.float32)  # noqa: E731
    q, k = quarters((rows, heads, d)), quarters((n, heads, d))
    q[:, :, 0] = np.sqrt(float(d))
    k[:, :, 0] = np.asarray(levels, np.float32)[:, None]
    return q.reshape(rows, heads * d), k.reshape(n, heads * d)
