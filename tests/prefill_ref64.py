"""Float64 reference of the prompt-route projection (launch_prefill_gemm) and its K-split rule, in plain numpy.

The attention reference is tests/decode_attention_ref64.attention64(..., causal_base=base): row s sees keys <= base + s."""
import numpy as np

from tests.decode_attention_ref64 import bf16_to_f64

PG_TILE, PG_BK = 64, 32


def gemm64(a, w, bias=None, r=None, gate=None, bf16=False):
    """y = a . w^T (+ bias) (+ r) in float64; w f32, or bf16 bit patterns widened exactly.  With `gate` the SwiGLU form: returns
    (y, gate / (1 + exp(-gate)) * y)."""
    w64 = bf16_to_f64(w) if bf16 else np.asarray(w, np.float64)
    y = np.asarray(a, np.float64) @ w64.T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)[None, :]
    if r is not None:
        y = y + np.asarray(r, np.float64)
    if gate is None:
        return y
    g = np.asarray(gate, np.float64)
    return y, g / (1.0 + np.exp(-g)) * y


def ksplit_rule(m, n, k, scratch=True):
    """The launcher's K-split rule restated: no split without a scratch or with n % 4; else doubling up to 8 slices while the
    launch stays within 1024 workgroups, the slices stay whole 32-wide K tiles and hold at least 128 columns of K."""
    if not scratch or n % 4:
        return 1
    tiles = -(-m // PG_TILE) * -(-n // PG_TILE)
    s = 1
    while s < 8 and tiles * s * 2 <= 1024 and k % (s * 2 * PG_BK) == 0 and k // (s * 2) >= 128:
        s *= 2
    return s


def geometry(m, n, k, scratch=True):
    """(ksplit, workgroups, K tiles per slice) of a launch."""
    s = ksplit_rule(m, n, k, scratch)
    return s, -(-m // PG_TILE) * -(-n // PG_TILE) * s, k // s // PG_BK
