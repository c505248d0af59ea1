"""Float64 reference of the FP8 prompt GEMM (launch_prefill_gemm_fp8) in plain numpy: the weights are decode(code) * scale with
the product taken in float64 (tests/fp8_fixture.TABLE and expand_scale), the rest is tests/prefill_ref64.gemm64.  The K-split
rule is prefill_ref64.ksplit_rule: the FP8 launcher takes prefill_gemm_launch_ksplit's answer."""
import numpy as np

from tests import fp8_fixture as F
from tests import prefill_ref64 as P

BAR = 1e-5   # the project's bar for FP8 projections: max |got - ref| <= BAR * max(1, max |ref|)


def weights64(codes, scale, kind):
    """decode(code) * scale, [n, k] float64 (an f32 scale times an e4m3 value is exact in float64)."""
    codes = np.asarray(codes, np.uint8)
    n, k = codes.shape
    return F.TABLE[codes].astype(np.float64) * F.expand_scale(np.asarray(scale, np.float32), kind, n, k).astype(np.float64)


def gemm64(a, codes, scale, kind, bias=None, r=None, gate=None):
    """y = a . (decode(codes) * scale)^T (+ bias) (+ r) in float64; with `gate`: (y, silu(gate) * y)."""
    return P.gemm64(a, weights64(codes, scale, kind), bias, r, gate)


def bar(ref):
    return BAR * max(1.0, float(np.abs(np.asarray(ref, np.float64)).max()))
