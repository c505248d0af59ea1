"""Compact lane KV caches on the GPU (lane_kv_kernels.hip): the encoding scatter and the grouped-query attention alone against
float64 (the decoders with bf16 / FP8 lanes: tests/test_gpu_lane_kv_models.py).

Bounds.  bf16 codes are held bit for bit to the round-to-nearest-even of the rows the f32 launcher stores (ops.wide_rope_scatter).
FP8: scale == amax / 448 to one f32 ulp, and |code * scale - x| <= 2^-4 |x| + 2^-10 scale: half a unit of a 3-bit mantissa plus
half a subnormal step.  Attention: 1e-5 * max(1, max |ref|) against float64 over the DECODED planes (tests/test_gpu_decode_attention.py's
bar)."""
import numpy as np
import pytest
import torch

from kjarni_amd import ops

pytestmark = pytest.mark.gpu
BF16, F8 = 1, 2
TYPES = [BF16, F8]


def _bf16_rne(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _decode(kv_type, codes, scales, d):
    """[lanes, rows, kv] codes (and [lanes, rows, kv_heads] scales) -> f32 values, as LlmModel::lane_kv_rows decodes them."""
    if kv_type == BF16:
        return (codes.astype(np.uint32) << 16).view(np.float32)
    vals = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).float().numpy()
    return vals * np.repeat(scales, d, axis=-1)


# ---- scatter ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rotate", "copy", "qwen3"])
@pytest.mark.parametrize("d,heads,kv_heads,lanes", [(16, 4, 4, 1), (64, 8, 2, 9), (128, 7, 1, 64)])
def test_scatter_against_the_f32_launcher(form, d, heads, kv_heads, lanes):
    rng = np.random.default_rng(d + lanes)
    cap, rows, kv = 6, 7, kv_heads * d
    qkv = rng.standard_normal((lanes, heads * d + 2 * kv + 4)).astype(np.float32)
    qkv[0, heads * d:heads * d + d] = 0.0                      # a K head row of zeros
    qkv[0, heads * d + kv + 3] = 64.0 * np.abs(qkv[0, heads * d + kv:heads * d + kv + d]).max()  # one V element 2^6 above its head
    pos = rng.integers(0, cap, lanes).astype(np.int32)
    live = np.ones(lanes, np.int32)
    pos[0] = 0
    if lanes > 1:
        pos[1], pos[2], live[3] = cap - 1, cap, 0              # the last row, a lane at its capacity, a frozen lane
    cos, sin = np.cos(rng.standard_normal((cap, d // 2))).astype(np.float32), np.sin(rng.standard_normal((cap, d // 2))).astype(np.float32)
    gam = dict(gamma_q=rng.standard_normal(d).astype(np.float32), gamma_k=rng.standard_normal(d).astype(np.float32), eps=1e-6) if form == "qwen3" else {}
    nan = np.full((lanes, rows, kv), np.nan, np.float32)
    q32, k32, v32 = ops.wide_rope_scatter(qkv, heads, kv_heads, d, cos, sin, nan, nan, cap, pos, live, rotate=form != "copy", **gam)
    wrote = np.array([bool(live[l]) and pos[l] < cap for l in range(lanes)])
    for kv_type in TYPES:
        dt, fill = (np.uint16, 0x7FC1) if kv_type == BF16 else (np.uint8, 0x7F)   # NaN codes in every element
        codes = np.full((lanes, rows, kv), fill, dt)
        scales = np.full((lanes, rows, kv_heads), np.nan, np.float32)
        q, kc, vc, ks, vs = ops.lane_kv_scatter(kv_type, qkv, heads, kv_heads, d, cos, sin, codes, codes, cap, pos, live, k_scale=scales,
                                                v_scale=scales, rotate=form != "copy", **gam)
        assert np.array_equal(q.view(np.uint32), q32.view(np.uint32)), "Q differs from the f32 launcher's"
        for name, got, gs, f32 in (("K", kc, ks, k32), ("V", vc, vs, v32)):
            for l in range(lanes):
                touched = np.zeros(rows, bool)
                if wrote[l]:
                    touched[pos[l]] = True
                assert (got[l, ~touched] == fill).all(), f"{name} lane {l}: a row it must not touch changed"
                if kv_type == F8:
                    assert np.isnan(gs[l, ~touched]).all(), f"{name} lane {l}: a scale it must not touch changed"
                if not wrote[l]:
                    continue
                x = f32[l, pos[l]]
                if kv_type == BF16:
                    assert np.array_equal(got[l, pos[l]], _bf16_rne(x)), f"{name} lane {l}: not RNE of the f32 row"
                    continue
                amax = np.abs(x.reshape(kv_heads, d)).max(axis=1)
                want = amax / np.float32(448.0)
                assert (np.abs(gs[l, pos[l]] - want) <= np.spacing(want)).all(), f"{name} lane {l}: scale"
                dec = _decode(F8, got[l:l + 1, pos[l]:pos[l] + 1], gs[l:l + 1, pos[l]:pos[l] + 1], d)[0, 0].astype(np.float64)
                bound = 2.0 ** -4 * np.abs(x.astype(np.float64)) + 2.0 ** -10 * np.repeat(gs[l, pos[l]].astype(np.float64), d)
                assert (np.abs(dec - x) <= bound).all(), f"{name} lane {l}: {np.abs(dec - x).max():.3e} outside the rounding bound"
                zero = amax == 0
                assert (gs[l, pos[l]][zero] == 0).all() and (got[l, pos[l]].reshape(kv_heads, d)[zero] == 0).all()


# ---- attention --------------------------------------------------------------------------------------------------------------------

def _ref_attention(q, K, V, heads, kv_heads, d, n):
    """float64 softmax(q K^T / sqrt d) V per lane over its first n[l] keys; zeros for an empty lane."""
    lanes, G = q.shape[0], heads // kv_heads
    out = np.zeros((lanes, heads * d))
    for l in range(lanes):
        if n[l] == 0:
            continue
        Kh, Vh = K[l, :n[l]].reshape(n[l], kv_heads, d).astype(np.float64), V[l, :n[l]].reshape(n[l], kv_heads, d).astype(np.float64)
        for h in range(heads):
            s = Kh[:, h // G] @ q[l, h * d:(h + 1) * d].astype(np.float64) / np.sqrt(d)
            p = np.exp(s - s.max())
            out[l, h * d:(h + 1) * d] = (p / p.sum()) @ Vh[:, h // G]
    return out


def _encode(kv_type, x, kv_heads, d):
    """Planes that hold representable values: bf16 by RNE; FP8 by torch's RNE convert of x / scale, scale = amax / 448."""
    if kv_type == BF16:
        return _bf16_rne(x).reshape(x.shape), None
    h = x.reshape(x.shape[:-1] + (kv_heads, d))
    scale = (np.abs(h).max(axis=-1) / 448.0).astype(np.float32)
    inv = np.where(scale > 0, 1.0 / np.where(scale > 0, scale, 1), 0).astype(np.float32)
    codes = torch.from_numpy(np.clip(h * inv[..., None], -448, 448).astype(np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return codes.reshape(x.shape), scale


@pytest.mark.parametrize("kv_type", TYPES, ids=["bf16", "fp8"])
@pytest.mark.parametrize("d,G,kv_heads,lanes,splits", [(16, 1, 3, 1, 1), (64, 3, 2, 9, 4), (128, 4, 2, 9, 4), (64, 7, 1, 64, 2), (128, 8, 1, 9, 3),
                                                       (32, 12, 2, 9, 4)])
def test_attention_against_float64(kv_type, d, G, kv_heads, lanes, splits):
    rng = np.random.default_rng(d * G + lanes)
    heads, kv, cap, rows = G * kv_heads, kv_heads * d, 41, 43
    # ragged: no key (pos 0 frozen is below), one key, either side of the splits * k boundaries of ceil(n / splits), the capacity
    edge = [0, splits - 1, splits, splits + 1, 2 * splits - 1, 2 * splits, 4 * splits, cap - 2, cap - 1, cap + 5]
    pos = np.array([edge[l % len(edge)] for l in range(lanes)], np.int32)
    live = np.ones(lanes, np.int32)
    if lanes > 1:
        live[lanes - 1] = 0
    n = np.where(live == 1, np.minimum(pos + 1, cap), 0)
    K, V = rng.standard_normal((lanes, rows, kv)).astype(np.float32), rng.standard_normal((lanes, rows, kv)).astype(np.float32)
    q = rng.standard_normal((lanes, heads * d)).astype(np.float32)
    if lanes > 2:
        q[1] = 0.0                                                       # Q = 0: the context is the mean of the decoded V
        K[2, :, :d] = 0.0                                                # exact scores of +-60 on head 0's keys: one element set
        K[2, ::2, 0], K[2, 1::2, 0], q[2, :d] = 1.0, -1.0, 0.0
        q[2, 0] = 60.0 * np.sqrt(d)
    kc, ks = _encode(kv_type, K, kv_heads, d)
    vc, vs = _encode(kv_type, V, kv_heads, d)
    Kd, Vd = _decode(kv_type, kc, ks, d), _decode(kv_type, vc, vs, d)
    ref = _ref_attention(q, Kd, Vd, heads, kv_heads, d, n)
    bad = 0x7FC1 if kv_type == BF16 else 0x7F                            # NaN behind every lane's last key; a frozen lane is all NaN
    for l in range(lanes):
        kc[l, n[l]:], vc[l, n[l]:] = bad, bad
        if ks is not None:
            ks[l, n[l]:], vs[l, n[l]:] = np.nan, np.nan
    got = ops.lane_attention_kv(kv_type, q, kc, vc, heads, kv_heads, d, cap, splits, pos, live, k_scale=ks, v_scale=vs)
    bar = 1e-5 * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print(f"largest error {err:.3e} = {err / bar:.3f} of the bar")
    assert np.isfinite(got).all() and err <= bar
    assert (got[n == 0] == 0).all()
    if lanes > 2:
        assert np.abs(got[1].reshape(heads, d) - Vd[1, :n[1]].reshape(n[1], kv_heads, d).astype(np.float64).mean(axis=0).repeat(G, axis=0)).max() <= bar
    again = ops.lane_attention_kv(kv_type, q, kc, vc, heads, kv_heads, d, cap, splits, pos, live, k_scale=ks, v_scale=vs)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "the same call twice gave other bits"
    if kv_type == BF16:                                                  # the f32 kernel on the widened copy agrees inside the bar
        stride = rows * kv
        f32 = ops.decode_attention(q, Kd, Vd, kv, kv, cap, heads, d, splits, kv_group=G, k_lane_stride=stride, v_lane_stride=stride, lanes=lanes,
                                   lane_pos=pos, lane_live=live)
        assert np.abs(f32.astype(np.float64) - got).max() <= bar

