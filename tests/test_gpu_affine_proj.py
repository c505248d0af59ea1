"""affine_kernels.hip alone, through kjarni_hip_op_affine_proj / _affine_dequant: the decode projection of Q4_0 / Q4_1 / Q5_0 / Q5_1 /
Q5_K (and Q8_0 beside them) against float64 over the host-dequantized weights, 1e-5 x max(1, |ref|); one-hot rows exact; every call
twice with the same bits; NaN wherever the kernel must neither read nor write.  K 2 080 / 2 304 span three LDS chunks of 1 024; from
32 768 columns (8 rows or SwiGLU: 16 384) a wave takes 4 (8 rows: 2) column pairs, the instances of a production head or gate / up."""
import ctypes as C

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import ops
from tests import gguf_fixture as G
from tests import gguf_types_fixture as T

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(T.NEW_TYPES)
KS = {n: ((256, 768, 2304) if n == "Q5_K" else (32, 896, 2080)) for n in NAMES}


def spread_blocks(t, n, k, rng):
    """Random blocks whose neighbouring runs (Q5_K: blocks) have a 2^6 apart and b of the other sign."""
    b = T.random_blocks(t, n, k, rng)
    v = b.reshape(-1, T.BLOCK.get(t, (32, 34))[1])
    odd = np.arange(v.shape[0]) % 2 == 1
    has_m = t in (T.Q4_1, T.Q5_1, T.Q5_K)   # m (Q5_K: dmin) sits behind d; else b = -8 d / -16 d changes sign with d
    for at, factor in ((0, 2.0 ** -6 if has_m else -(2.0 ** -6)),) + (((2, -1.0),) if has_m else ()):
        f = v[:, at:at + 2].copy().view(np.float16)[:, 0].astype(F32)
        f[odd] *= factor
        v[:, at:at + 2] = f.astype(np.float16).view(np.uint8).reshape(-1, 2)
    return b


def nans(r, c):
    return np.full((r, c), np.nan, F32)


def rows_x(rows, k, rng, pad=4):
    """x [rows + 1, k + pad]: the row behind the last and the columns behind k are NaN."""
    x = nans(rows + 1, k + pad)
    x[:rows, :k] = rng.standard_normal((rows, k)).astype(F32)
    return x


def close(got, ref):
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref).max()
    assert err <= 1e-5 * max(1.0, np.abs(ref).max()), err


def twice(call):
    a, b = call(), call()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    return a


@pytest.mark.parametrize("name,k", [(n, k) for n in NAMES for k in KS[n]])
def test_plain_bias_and_in_place_residual(name, k):
    t, rng = T.NEW_TYPES[name], np.random.default_rng(k)
    for n in (2, 7, 130) + ((32768 + 13,) if k == KS[name][0] else ()):
        blocks = spread_blocks(t, n, k, rng)
        w = T.dequantize(t, blocks, n, k).astype(np.float64)
        bias = rng.standard_normal(n + 5).astype(F32)
        for rows in (1, 3, 8):
            x = rows_x(rows, k, rng)
            y = nans(rows + 2, n + 3)
            y[:rows, :n] = rng.standard_normal((rows, n)).astype(F32)
            ref = x[:rows, :k].astype(np.float64) @ w.T + bias[5:5 + n] + y[:rows, :n]
            (got,) = twice(lambda: ops.affine_proj(0, [(t, blocks)], x, rows, [y], bias=bias, bias_off=(5, 0, 0), r_is_y0=True, k=k))
            close(got[:rows, :n], ref)
            assert np.isnan(got[rows:]).all() and np.isnan(got[:, n:]).all()


AT = (0, 15, 16, 31)   # the nibble boundary and the ends of a run


def fifth_bits_alone(t, blocks):
    """5-bit types: every nibble zero, the fifth bit set at the elements AT of every run and nowhere else."""
    at = {T.Q5_0: 2, T.Q5_1: 4, T.Q5_K: 16}[t]
    v = blocks.reshape(-1, T.BLOCK[t][1])
    v[:, at:] = 0
    if t == T.Q5_K:
        v[:, [at + e for e in AT]] = 0xFF   # (qh byte e: bit j is sub-block j's element e)
    else:
        v[:, at:at + 4] = np.array([sum(1 << e for e in AT)], "<u4").view(np.uint8)


@pytest.mark.parametrize("name", NAMES)
def test_one_hot_rows_give_the_weight_itself(name):
    t, rng = T.NEW_TYPES[name], np.random.default_rng(5)
    n, k, at = 7, (256 if name == "Q5_K" else 96), AT
    blocks = spread_blocks(t, n, k, rng)
    if name in ("Q5_0", "Q5_1", "Q5_K"):
        fifth_bits_alone(t, blocks)
    w = T.dequantize(t, blocks, n, k)
    x = np.zeros((4, k), F32)
    for r, e in enumerate(at):
        x[r, 32 + e] = 1.0
    (got,) = twice(lambda: ops.affine_proj(0, [(t, blocks)], x, 4, [nans(4, n)], k=k))
    want = np.stack([w[:, 32 + e] for e in at])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_qkv_three_types_at_a_row_offset(name):
    t, k, off = T.NEW_TYPES[name], KS[name][1], 3
    rng = np.random.default_rng(11)
    other = T.Q4_1 if name != "Q4_1" else T.Q5_0
    mats = [(t, spread_blocks(t, 70, k, rng)), (8, spread_blocks(8, 9, k, rng)), (other, spread_blocks(other, 6, k, rng))]
    ws = [T.dequantize(tt, b, b.shape[0], k).astype(np.float64) for tt, b in mats]
    bias = rng.standard_normal(100).astype(F32)
    boff = (7, 80, 90)
    gamma = (1.0 + 0.1 * rng.standard_normal(k)).astype(F32)
    for rows in (1, 3, 8):
        x = rows_x(rows, k, rng)
        xs = x[:rows, :k].astype(np.float64)
        xn = xs / np.sqrt((xs ** 2).mean(axis=1, keepdims=True) + 1e-5) * gamma
        for on_device in (False, True):
            ys = [nans(rows, 71), nans(rows + off + 2, 11), nans(rows + off + 2, 6)]
            got = twice(lambda: ops.affine_proj(1, mats, x, rows, ys, gamma=gamma, eps=1e-5, bias=bias, bias_off=boff, row_off=off,
                                                offset_on_device=on_device, k=k))
            for i, (g, w) in enumerate(zip(got, ws)):
                base, n = (0 if i == 0 else off), w.shape[0]
                close(g[base:base + rows, :n], xn @ w.T + bias[boff[i]:boff[i] + n])
                g[base:base + rows, :n] = np.nan
                assert np.isnan(g).all()


@pytest.mark.parametrize("name", NAMES)
def test_swiglu(name):
    t, rng = T.NEW_TYPES[name], np.random.default_rng(13)
    for up_t, n, k in ((t, 37, KS[name][1]), (8, 37, KS[name][1]), (t, 16384 + 5, KS[name][0])):   # one width; two; the wider instances
        gate, up = spread_blocks(t, n, k, rng), spread_blocks(up_t, n, k, rng)
        wg, wu = T.dequantize(t, gate, n, k).astype(np.float64), T.dequantize(up_t, up, n, k).astype(np.float64)
        for rows in (1, 3, 8):
            x = rows_x(rows, k, rng)
            g, u = x[:rows, :k].astype(np.float64) @ wg.T, x[:rows, :k].astype(np.float64) @ wu.T
            (got,) = twice(lambda: ops.affine_proj(2, [(t, gate), (up_t, up)], x, rows, [nans(rows + 1, n + 1)], k=k))
            close(got[:rows, :n], g / (1.0 + np.exp(-g)) * u)
            assert np.isnan(got[rows:]).all() and np.isnan(got[:, n:]).all()


@pytest.mark.parametrize("name", NAMES)
def test_dequant_and_embed_equal_the_host_reader(tmp_path, name):
    t, n, k = T.NEW_TYPES[name], 9, 768
    blocks = T.random_blocks(t, n, k, np.random.default_rng(t))
    path = G.write_gguf(str(tmp_path / "one.gguf"), {"general.architecture": "qwen2"}, [("blk.0.attn_v.weight", t, (k, n), blocks)])
    host = np.empty(n * k, F32)
    size, shape, nd = C.c_size_t(), (C.c_int64 * 2)(), C.c_int32()
    assert kjarni_amd.lib().kjarni_gguf_tensor_f32(path.encode(), b"model.layers.0.self_attn.v_proj.weight",
                                                   host.ctypes.data_as(C.POINTER(C.c_float)), host.size, C.byref(size), shape, C.byref(nd)) == 0
    host = host.reshape(n, k)
    assert np.array_equal(ops.affine_dequant(t, blocks, n, k).view(np.uint32), host.view(np.uint32))
    ids = [8, 0, n, 3, 2 ** 31]
    rows = ops.affine_dequant(t, blocks, n, k, ids=ids)
    want = np.stack([host[i] if i < n else np.zeros(k, F32) for i in ids])
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))
