"""Single operators of the forward pass on host arrays (kjarni_hip.h, "single operators"):
the reference's LinearLayer::matmul (+ fused epilogue), EncoderSelfAttention core and
LayerNorm::forward, each as one HIP kernel.  For parity tests and micro-benchmarks."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _ffi
from ._ffi import check_error, lib

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GELU_NEW, EPI_BIAS_RELU, EPI_BIAS_TANH, EPI_BIAS_RESIDUAL, EPI_BIAS_MUL_SILU = range(7)
POOL_MEAN, POOL_CLS, POOL_MAX, POOL_LAST = 0, 1, 2, 3


def _f(a):
    return None if a is None else a.ctypes.data_as(_ffi._f32p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def linear(x, w, bias=None, residual=None, epilogue: int = EPI_BIAS, iters: int = 0, device: int = 0
           ) -> Tuple[np.ndarray, Optional[float]]:
    x, w, bias, residual = _c(x), _c(w), _c(bias), _c(residual)
    m, k = x.shape
    n = w.shape[0]
    y = np.empty((m, n), np.float32)
    ms = C.c_float(0)
    check_error(lib().kjarni_hip_op_linear(device, _f(x), _f(w), _f(bias), _f(residual), m, k, n, epilogue, _f(y),
                                           iters, C.byref(ms)))
    return y, (float(ms.value) if iters > 0 else None)


def to_bf16(w: np.ndarray) -> np.ndarray:
    """f32 -> bf16 bit patterns (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(w, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(w16: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(w16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def linear_bf16_weights(x, w_bf16, bias=None, residual=None, epilogue: int = EPI_BIAS, iters: int = 0, device: int = 0
                        ) -> Tuple[np.ndarray, Optional[float]]:
    """y = epilogue(x . w^T + bias (+ residual)) with w given as bf16 bit patterns [n, k] (kjarni_hip_op_linear_bf16_weights)."""
    x, bias, residual = _c(x), _c(bias), _c(residual)
    w16 = np.ascontiguousarray(w_bf16, np.uint16)
    m, k = x.shape
    n = w16.shape[0]
    y = np.empty((m, n), np.float32)
    ms = C.c_float(0)
    check_error(lib().kjarni_hip_op_linear_bf16_weights(device, _f(x), w16.ctypes.data_as(C.c_void_p), _f(bias), _f(residual), m, k, n,
                                                        epilogue, _f(y), iters, C.byref(ms)))
    return y, (float(ms.value) if iters > 0 else None)


def attention(qkv, mask, heads: int, mask_value: float = -1e9, iters: int = 0, device: int = 0
              ) -> Tuple[np.ndarray, Optional[float]]:
    qkv = _c(qkv)
    b, s, h3 = qkv.shape
    hidden = h3 // 3
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    ctx = np.empty((b, s, hidden), np.float32)
    ms = C.c_float(0)
    check_error(lib().kjarni_hip_op_attention(device, _f(qkv), None if mask is None else mask.ctypes.data_as(_ffi._u32p),
                                              b, s, heads, hidden // heads, float(mask_value), _f(ctx), iters,
                                              C.byref(ms)))
    return ctx, (float(ms.value) if iters > 0 else None)


def pool(hidden_states, mask=None, pooling: int = 0, normalize: bool = False, device: int = 0) -> np.ndarray:
    """hidden_states [B, S, H] -> [B, H] (kjarni_hip_op_pool): pooling 0 mean, 1 cls, 2 max, 3 last token; optional L2."""
    h = _c(hidden_states)
    b, s, d = h.shape
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    out = np.empty((b, d), np.float32)
    check_error(lib().kjarni_hip_op_pool(device, _f(h), None if mask is None else mask.ctypes.data_as(_ffi._u32p), b, s, d,
                                         int(pooling), 1 if normalize else 0, _f(out)))
    return out


def attention_biased(qkv, mask, heads: int, position_bias=None, scale_qk: bool = True, mask_value: float = -1e9,
                     device: int = 0) -> np.ndarray:
    """EncoderSelfAttention with the reference's full argument list (kjarni_hip_op_attention_biased): position_bias
    [1, heads, S', S'] or [heads, S', S'] with S' >= seq, added after the scale and before the padding mask."""
    qkv = _c(qkv)
    b, s, h3 = qkv.shape
    hidden = h3 // 3
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint32)
    bias, bias_seq = None, 0
    if position_bias is not None:
        bias = np.ascontiguousarray(position_bias, np.float32)
        bias = bias.reshape(bias.shape[-3:])
        assert bias.shape[0] == heads and bias.shape[1] == bias.shape[2]
        bias_seq = int(bias.shape[1])
    ctx = np.empty((b, s, hidden), np.float32)
    check_error(lib().kjarni_hip_op_attention_biased(device, _f(qkv), None if mask is None else mask.ctypes.data_as(_ffi._u32p),
                                                     None if bias is None else _f(bias), bias_seq, b, s, heads, hidden // heads,
                                                     1 if scale_qk else 0, float(mask_value), _f(ctx)))
    return ctx


def layer_norm(x, gamma, beta, eps: float, iters: int = 0, device: int = 0) -> Tuple[np.ndarray, Optional[float]]:
    x, gamma, beta = _c(x), _c(gamma), _c(beta)
    hidden = x.shape[-1]
    rows = x.size // hidden
    y = np.empty_like(x)
    ms = C.c_float(0)
    check_error(lib().kjarni_hip_op_layer_norm(device, _f(x), _f(gamma), _f(beta), float(eps), rows, hidden, _f(y),
                                               iters, C.byref(ms)))
    return y, (float(ms.value) if iters > 0 else None)


def linear_layer_norm(x, w, bias, residual, gamma, beta, eps: float, iters: int = 0, device: int = 0
                      ) -> Tuple[np.ndarray, Optional[float]]:
    """LayerNorm(x . w^T + bias + residual) * gamma + beta (kjarni_hip_op_linear_layer_norm)."""
    x, w, bias, residual, gamma, beta = _c(x), _c(w), _c(bias), _c(residual), _c(gamma), _c(beta)
    m, k = x.shape
    n = w.shape[0]
    y = np.empty((m, n), np.float32)
    ms = C.c_float(0)
    check_error(lib().kjarni_hip_op_linear_layer_norm(device, _f(x), _f(w), _f(bias), _f(residual), _f(gamma), _f(beta),
                                                      float(eps), m, k, n, _f(y), iters, C.byref(ms)))
    return y, (float(ms.value) if iters > 0 else None)


def set_f32_on_bf16(on: bool) -> bool:
    """Process-wide opt-in (kjarni_hip_set_f32_on_bf16): the large-batch projections compute their f32 products on the bf16
    matrix cores from three exact bf16 pieces per operand.  Returns the previous setting."""
    return bool(lib().kjarni_hip_set_f32_on_bf16(1 if on else 0))


def clock_probe(out_dev_ptr: int, spin_us: int = 20, stream: int = 0) -> None:
    """Enqueues the one-wave clock probe (kjarni_hip_clock_probe): out_dev_ptr -> two uint64 on the device, [shader cycles,
    10 ns ticks]; GHz = cycles / ticks / 10."""
    check_error(lib().kjarni_hip_clock_probe(out_dev_ptr, int(spin_us), stream))


def clock_trace(out_dev_ptr: int, samples: int, window_us: int, stream: int) -> None:
    """Enqueues the repeated clock reading (kjarni_hip_clock_trace) on `stream` -- a stream of its own beside the work being
    measured: out_dev_ptr -> samples x [shader cycles, 10 ns ticks] uint64 on the device."""
    check_error(lib().kjarni_hip_clock_trace(out_dev_ptr, int(samples), int(window_us), stream))


def measurement_stream() -> int:
    """The library's own non-blocking stream for clock traces (kjarni_hip_measurement_stream); 0 if it cannot be made."""
    return int(lib().kjarni_hip_measurement_stream() or 0)


def measurement_stream_release() -> None:
    """Waits for the measurement stream and destroys it (kjarni_hip_measurement_stream_release)."""
    lib().kjarni_hip_measurement_stream_release()


def get_f32_on_bf16() -> bool:
    return bool(lib().kjarni_hip_get_f32_on_bf16())


def lookup_draft(tokens, draft_tokens: int = 7, ngram_max: int = 3, ngram_min: int = 1, device: Optional[int] = 0):
    """The prompt-lookup draft after the history `tokens` (a list of ids): the device kernel, or with device=None the host
    restatement of the same rule."""
    t = np.ascontiguousarray(tokens, np.uint32)
    cfg = _ffi.KjarniHipLookupConfig(draft_tokens, ngram_max, ngram_min)
    out = np.zeros(8, np.uint32)
    n = C.c_int32(0)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    if device is None:
        check_error(lib().kjarni_lookup_draft(u32(t), t.size, C.byref(cfg), u32(out), C.byref(n)))
    else:
        check_error(lib().kjarni_hip_op_lookup_draft(device, u32(t), t.size, C.byref(cfg), u32(out), C.byref(n)))
    return out[:n.value].tolist()


def kv_prefix_copy(src, dst, dst_offset: int, count: int, src_skew: int = 0, dst_skew: int = 0, device: int = 0):
    """The lanes' shared-prefix copy kernel alone: src [2 * layers, src_floats], dst [2 * layers, dst_floats]; returns dst with
    src[c, :count] at dst[c, dst_offset:dst_offset + count] for every cache c.  The skews (0..3 floats) move the device
    buffers off their 16-byte boundaries."""
    s, d = np.ascontiguousarray(src, np.float32), np.array(dst, np.float32, order="C")
    if s.ndim != 2 or d.ndim != 2 or s.shape[0] != d.shape[0] or s.shape[0] % 2:
        raise ValueError("src and dst: [2 * layers, floats]")
    f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check_error(lib().kjarni_hip_op_kv_prefix_copy(device, f(s), s.shape[0] // 2, s.shape[1], src_skew, d.shape[1], dst_skew, int(dst_offset),
                                                   int(count), f(d)))
    return d


def qk_norm_rope(q, k, rows: int, n_heads: int, n_kv_heads: int, head_dim: int, gamma_q, gamma_k, eps: float, cos, sin, pos: int,
                 pos_on_device: bool = False, k_at_cache_row: bool = False, device: int = 0):
    """Qwen3's per-head RMSNorm + RoPE kernel alone: q [q_rows, ldq] and k [k_rows, ldk] (leading dimensions may exceed the
    used widths) -> (q, k) after the call on `rows` rows at base position `pos`; cos / sin [table_rows, head_dim // 2].
    K row r is row pos + r of k when k_at_cache_row, else row r."""
    qa, ka = np.array(q, np.float32, order="C"), np.array(k, np.float32, order="C")
    gq, gk = np.ascontiguousarray(gamma_q, np.float32), np.ascontiguousarray(gamma_k, np.float32)
    ct, st = np.ascontiguousarray(cos, np.float32), np.ascontiguousarray(sin, np.float32)
    if qa.ndim != 2 or ka.ndim != 2 or gq.shape != (head_dim,) or gk.shape != (head_dim,):
        raise ValueError("q and k: [rows, ld]; gammas: [head_dim]")
    if ct.ndim != 2 or ct.shape != st.shape or ct.shape[1] != head_dim // 2:
        raise ValueError("cos and sin: [table_rows, head_dim // 2]")
    f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    check_error(lib().kjarni_hip_op_qk_norm_rope(device, f(qa), qa.shape[1], qa.shape[0], f(ka), ka.shape[1], ka.shape[0], int(rows),
                                                 int(n_heads), int(n_kv_heads), int(head_dim), f(gq), f(gk), float(eps), f(ct), f(st),
                                                 ct.shape[0], int(pos), int(bool(pos_on_device)), int(bool(k_at_cache_row))))
    return qa, ka


ARGMAX_DECODER, ARGMAX_LANES, ARGMAX_LOOKUP = 0, 1, 2
_i32p = C.POINTER(C.c_int32)


# ---- decoder embedders: the packed-row kernels alone ----
def _seq_start(lengths):
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]), np.int32)


def packed_causal_attention(q, k, v, lengths, heads: int, kv_heads: int, head_dim: int, ctx=None, device: int = 0):
    """Causal grouped-query attention over packed sequences: q [rows, ldq], k / v [rows, ldk / ldv] hold the sequences of
    `lengths` one after another from row 0 (rows may exceed their total, leading dimensions the used widths).  Returns ctx
    [rows, ldc] (given, or zeros [rows, heads * head_dim]) with the context rows written; everything else as it was."""
    qa, ka, va = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
    ca = np.zeros((qa.shape[0], heads * head_dim), np.float32) if ctx is None else np.array(ctx, np.float32, order="C")
    if any(x.ndim != 2 or x.shape[0] != qa.shape[0] for x in (qa, ka, va, ca)):
        raise ValueError("q, k, v, ctx: [rows, ld] with the same rows")
    st = _seq_start(lengths)
    check_error(lib().kjarni_hip_op_packed_causal_attention(device, _f(qa), qa.shape[1], _f(ka), ka.shape[1], _f(va), va.shape[1], qa.shape[0],
                                                            st.ctypes.data_as(_i32p), st.size - 1, int(heads), int(kv_heads), int(head_dim),
                                                            _f(ca), ca.shape[1]))
    return ca


# ---- the decode attention and the projections that merge its slabs, alone ----
def decode_attention(q, k, v, ldk: int, ldv: int, n_keys: int, heads: int, head_dim: int, splits: int, causal_base: int = -1,
                     kv_group: int = 1, keys_on_device: bool = False, max_keys: int = 0, k_lane_stride: int = 0, v_lane_stride: int = 0,
                     lanes: int = 0, lane_pos=None, lane_live=None, ctx=None, want_slabs: bool = False, device: int = 0):
    """launch_decode_attention on host arrays (kjarni_hip_op_decode_attention).  q [rows, ldq]; k and v are flat float buffers the
    caller lays out itself (key row t of query row s at s * lane stride + t * ldk).  Returns ctx [rows, ldc] (given, or NaN
    [rows, heads * head_dim]) with the context rows written and, with want_slabs, the scratch [rows, heads, splits, head_dim + 4]."""
    qa = np.ascontiguousarray(q, np.float32)
    ka, va = np.ascontiguousarray(k, np.float32).reshape(-1), np.ascontiguousarray(v, np.float32).reshape(-1)
    if qa.ndim != 2:
        raise ValueError("q: [rows, ldq]")
    rows = qa.shape[0]
    ca = np.full((rows, heads * head_dim), np.nan, np.float32) if ctx is None else np.array(ctx, np.float32, order="C")
    if ca.ndim != 2 or ca.shape[0] != rows:
        raise ValueError("ctx: [rows, ldc]")
    pos = None if lane_pos is None else np.ascontiguousarray(lane_pos, np.int32)
    live = None if lane_live is None else np.ascontiguousarray(lane_live, np.int32)
    if any(x is not None and x.shape != (rows,) for x in (pos, live)):
        raise ValueError("lane_pos / lane_live: [rows]")
    sl = np.empty((rows, heads, max(int(splits), 0), head_dim + 4), np.float32) if want_slabs else None
    p = lambda x: None if x is None else x.ctypes.data_as(_i32p)  # noqa: E731
    check_error(lib().kjarni_hip_op_decode_attention(device, _f(qa), qa.shape[1], rows, _f(ka), ka.size, int(ldk), _f(va), va.size, int(ldv),
                                                     int(n_keys), int(bool(keys_on_device)), int(max_keys), int(heads), int(head_dim),
                                                     int(causal_base), int(splits), int(kv_group), int(k_lane_stride), int(v_lane_stride),
                                                     int(lanes), p(pos), p(live), _f(ca), ca.shape[1], _f(sl)))
    return (ca, sl) if want_slabs else ca


def _slab_args(slabs, w, bias, r, head_dim):
    sa = np.ascontiguousarray(slabs, np.float32)
    if sa.ndim != 3 or sa.shape[2] != head_dim + 4 or w.ndim != 2 or w.shape[1] != sa.shape[0] * head_dim:
        raise ValueError("slabs: [heads, splits, head_dim + 4]; w: [n_out, heads * head_dim]")
    n_out = w.shape[0]
    ba, ra = (None if x is None else np.ascontiguousarray(x, np.float32) for x in (bias, r))
    if any(x is not None and x.shape != (n_out,) for x in (ba, ra)):
        raise ValueError("bias / r: [n_out]")
    return sa, ba, ra, n_out


def gemv_row_att(slabs, w, bias, r, head_dim: int, in_place: bool = False, two_step: bool = False, device: int = 0):
    """y [n_out] = merged(slabs) . w^T + bias + r by launch_gemv_row_att (kjarni_hip_op_gemv_row_att); two_step: by the combine
    pass and the one-row projection instead.  slabs [heads, splits, head_dim + 4], w [n_out, heads * head_dim]."""
    wa = np.ascontiguousarray(w, np.float32)
    sa, ba, ra, n_out = _slab_args(slabs, wa, bias, r, head_dim)
    y = np.full(n_out, np.nan, np.float32)
    check_error(lib().kjarni_hip_op_gemv_row_att(device, _f(sa), sa.shape[1], int(head_dim), _f(wa), _f(ba), _f(ra), n_out, wa.shape[1],
                                                 int(bool(in_place)), int(bool(two_step)), _f(y)))
    return y


def llm_gemv_att(slabs, w, bias, r, head_dim: int, bf16: bool = False, rows: int = 1, device: int = 0):
    """The same through launch_llm_gemv's slab-merging branch (kjarni_hip_op_llm_gemv_att); w f32, or bf16 bit patterns
    (uint16) with bf16 = True."""
    wa = np.ascontiguousarray(w, np.uint16 if bf16 else np.float32)
    sa, ba, ra, n_out = _slab_args(slabs, wa, bias, r, head_dim)
    y = np.full(n_out, np.nan, np.float32)
    check_error(lib().kjarni_hip_op_llm_gemv_att(device, _f(sa), sa.shape[1], int(head_dim), wa.ctypes.data_as(C.c_void_p), int(bool(bf16)),
                                                 _f(ba), _f(ra), n_out, wa.shape[1], int(rows), _f(y)))
    return y


# ---- the prompt-route GEMM and the two prefill attention kernels, alone ----
def prefill_gemm(a, w, m: int, y, bias=None, r=None, r_is_y: bool = False, gate=None, bf16: bool = False, split: bool = True,
                 want_scratch_written: bool = False, device: int = 0):
    """launch_prefill_gemm on host arrays (kjarni_hip_op_prefill_gemm): a [a_rows, lda] (k = w's width used), w [n, k] f32 or bf16
    bit patterns (uint16, bf16 = True), y [m, ldy] given with whatever its padding holds, r [m, ldr] or r_is_y (the residual is y),
    gate [m, n].  Returns (y, gate or None, ksplit_used[, scratch words written]) -- copies; the arguments stay as they were."""
    aa = np.ascontiguousarray(a, np.float32)
    wa = np.ascontiguousarray(w, np.uint16 if bf16 else np.float32)
    ya = np.array(y, np.float32, order="C")
    if aa.ndim != 2 or wa.ndim != 2 or ya.ndim != 2 or ya.shape[0] != int(m):
        raise ValueError("a: [a_rows, lda]; w: [n, k]; y: [m, ldy]")
    n, k = wa.shape
    ba = _proj_vector(bias, n, "bias")
    ra = None if r is None else np.ascontiguousarray(r, np.float32)
    if ra is not None and (ra.ndim != 2 or ra.shape[0] != int(m)):
        raise ValueError("r: [m, ldr]")
    ga = None if gate is None else np.array(gate, np.float32, order="C")
    if ga is not None and ga.shape != (int(m), n):
        raise ValueError("gate: [m, n]")
    used, written = C.c_int32(-1), C.c_int64(-1)
    check_error(lib().kjarni_hip_op_prefill_gemm(device, _f(aa), aa.shape[1], aa.shape[0], wa.ctypes.data_as(C.c_void_p), int(bool(bf16)), _f(ba),
                                                 _f(ra), 0 if ra is None else ra.shape[1], int(bool(r_is_y)), _f(ya), ya.shape[1], _f(ga), int(m),
                                                 n, k, int(bool(split)), C.byref(used), C.byref(written) if want_scratch_written else None))
    return (ya, ga, used.value, written.value) if want_scratch_written else (ya, ga, used.value)


def prefill_gemm_fp8(a, codes, scale, m: int, y, bias=None, r=None, r_is_y: bool = False, gate=None, split: bool = True,
                     want_scratch_written: bool = False, device: int = 0):
    """launch_prefill_gemm_fp8 on host arrays (kjarni_hip_op_prefill_gemm_fp8): prefill_gemm's arguments with the weights as FP8
    (e4m3fn) codes [n, k] (uint8) and their scales [scale_rows, scale_cols] (2-D: [1, 1], [n, 1] or [ceil(n / 128), k / 128]).
    Returns (y, gate or None, ksplit_used[, scratch words written]) -- copies; the arguments stay as they were."""
    aa = np.ascontiguousarray(a, np.float32)
    ca = np.ascontiguousarray(codes, np.uint8)
    sa = np.ascontiguousarray(scale, np.float32)
    ya = np.array(y, np.float32, order="C")
    if aa.ndim != 2 or ca.ndim != 2 or sa.ndim != 2 or ya.ndim != 2 or ya.shape[0] != int(m):
        raise ValueError("a: [a_rows, lda]; codes: [n, k]; scale: [scale_rows, scale_cols]; y: [m, ldy]")
    n, k = ca.shape
    ba = _proj_vector(bias, n, "bias")
    ra = None if r is None else np.ascontiguousarray(r, np.float32)
    if ra is not None and (ra.ndim != 2 or ra.shape[0] != int(m)):
        raise ValueError("r: [m, ldr]")
    ga = None if gate is None else np.array(gate, np.float32, order="C")
    if ga is not None and ga.shape != (int(m), n):
        raise ValueError("gate: [m, n]")
    used, written = C.c_int32(-1), C.c_int64(-1)
    check_error(lib().kjarni_hip_op_prefill_gemm_fp8(device, _f(aa), aa.shape[1], aa.shape[0], ca.ctypes.data_as(C.c_void_p), _f(sa), sa.shape[0],
                                                     sa.shape[1], _f(ba), _f(ra), 0 if ra is None else ra.shape[1], int(bool(r_is_y)), _f(ya),
                                                     ya.shape[1], _f(ga), int(m), n, k, int(bool(split)), C.byref(used),
                                                     C.byref(written) if want_scratch_written else None))
    return (ya, ga, used.value, written.value) if want_scratch_written else (ya, ga, used.value)


# ---- the dense (f32 / bf16) decode-step projections, alone ----
GEMV_STREAM, GEMV_SPLITK, GEMV_ONE, GEMV_GENERIC = 0, 1, 2, 3
QKV_PAIR, QKV_STREAM, QKV_STREAM_EMBED = 0, 1, 2


def llm_gemv(x, w, rows: int, ys, k: Optional[int] = None, lanes: bool = False, gamma=None, beta=None, eps: float = 0.0,
             layernorm: bool = False, gelu_tanh: bool = False, w2=None, bf16: bool = False, swiglu: bool = False, bias=None, r=None,
             r_is_y0: bool = False, seg_q: int = 0, seg_kv: int = 0, row_off: int = 0, offset_on_device: bool = False, norm_out=None,
             device: int = 0):
    """One launch_llm_gemv (lanes: launch_llm_gemv_lanes) on host arrays (kjarni_hip_op_llm_gemv).  x [x_rows, ldx] (k = w's width
    unless given); w, w2 [n_out, k] f32 or bf16 bit patterns (uint16, bf16 = True); ys: 1 or 3 outputs [out_rows, ldy] as they are
    before the launch (seg_q > 0: Q, K, V; the two caches share their stride); r [rows, ldr] or r_is_y0; norm_out [k] as it is
    before the launch.  Returns (outputs, norm_out or None, route) -- copies; route is a dict of the launcher's own decisions."""
    xa = np.ascontiguousarray(x, np.float32)
    wa = np.ascontiguousarray(w, np.uint16 if bf16 else np.float32)
    w2a = None if w2 is None else np.ascontiguousarray(w2, np.uint16 if bf16 else np.float32)
    out = [np.array(y, np.float32, order="C") for y in ys]
    if xa.ndim != 2 or wa.ndim != 2 or len(out) not in (1, 3) or any(y.ndim != 2 for y in out) or (w2a is not None and w2a.shape != wa.shape):
        raise ValueError("x: [x_rows, ldx]; w, w2: [n_out, k]; ys: 1 or 3 arrays [out_rows, ldy]")
    if len(out) == 3 and out[1].shape[1] != out[2].shape[1]:
        raise ValueError("ys[1] and ys[2] share ldy12")
    n_out = wa.shape[0]
    kk = wa.shape[1] if k is None else int(k)
    g, be, b = _proj_vector(gamma, kk, "gamma"), _proj_vector(beta, kk, "beta"), _proj_vector(bias, n_out, "bias")
    ra = None if r is None else np.ascontiguousarray(r, np.float32)
    if ra is not None and (ra.ndim != 2 or ra.shape[0] < max(int(rows), 1)):
        raise ValueError("r: [rows, ldr]")
    no = None if norm_out is None else np.array(norm_out, np.float32, order="C")
    if no is not None and no.size != kk:
        raise ValueError("norm_out: [k]")
    yp = (C.c_void_p * 3)(*[y.ctypes.data for y in out])
    orows = (C.c_int32 * 3)(*[y.shape[0] for y in out])
    route = (C.c_int32 * 16)(*([-1] * 16))
    v = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)  # noqa: E731
    check_error(lib().kjarni_hip_op_llm_gemv(device, int(bool(lanes)), _f(xa), xa.shape[0], xa.shape[1], int(rows), _f(g), _f(be), float(eps),
                                             int(bool(layernorm)), int(bool(gelu_tanh)), v(wa), v(w2a), int(bool(bf16)), int(bool(swiglu)), _f(b),
                                             _f(ra), 0 if ra is None else ra.shape[1], int(bool(r_is_y0)), n_out, kk, int(seg_q), int(seg_kv), yp,
                                             orows, out[0].shape[1], out[1].shape[1] if len(out) == 3 else 0, int(row_off),
                                             int(bool(offset_on_device)), _f(no), route))
    names = ("taken", "ch", "ns", "wide", "cpw", "workgroups", "streamed") if lanes else \
        ("kernel", "ch", "wide", "threads", "loop", "rows_per_batch", "workgroups")
    rt = dict(zip(names, list(route)[:7]))
    if lanes and not rt["taken"]:
        rt["fallback"] = dict(zip(("kernel", "ch", "wide", "threads", "loop", "rows_per_batch", "workgroups"), list(route)[8:15]))
    return out, no, rt


def llm_qkv_rope(w, gamma, n_heads: int, n_kv_heads: int, head_dim: int, cos_t, sin_t, pos: int, q, k_cache, v_cache, x=None,
                 embed_id: Optional[int] = None, table=None, eps: float = 0.0, bf16: bool = False, bias=None, offset_on_device: bool = False,
                 x_raw_out=None, device: int = 0):
    """One launch_llm_qkv_rope on host arrays (kjarni_hip_op_llm_qkv_rope).  x [k], or embed_id with table [vocab, k] (the weights'
    dtype); w [(n_heads + 2 n_kv_heads) * head_dim, k]; cos_t / sin_t [positions, head_dim / 2]; q [n_heads * head_dim], k_cache /
    v_cache [cache_rows, n_kv_heads * head_dim] and x_raw_out [k] as they are before the launch.  Returns (q, k_cache, v_cache,
    x_raw_out or None, route) -- copies; route is a dict of the launcher's own decisions."""
    wt = np.uint16 if bf16 else np.float32
    wa = np.ascontiguousarray(w, wt)
    if wa.ndim != 2 or wa.shape[0] != (int(n_heads) + 2 * int(n_kv_heads)) * int(head_dim):
        raise ValueError("w: [(n_heads + 2 n_kv_heads) * head_dim, k]")
    kk = wa.shape[1]
    xa = _proj_vector(x, kk, "x")
    ta = None if table is None else np.ascontiguousarray(table, wt)
    if ta is not None and (ta.ndim != 2 or ta.shape[1] != kk):
        raise ValueError("table: [vocab, k]")
    ida = None if embed_id is None else np.array([int(embed_id)], np.uint32)
    g, b = _proj_vector(gamma, kk, "gamma"), _proj_vector(bias, wa.shape[0], "bias")
    ca, sa = np.ascontiguousarray(cos_t, np.float32), np.ascontiguousarray(sin_t, np.float32)
    if ca.ndim != 2 or ca.shape != sa.shape or ca.shape[1] != int(head_dim) // 2:
        raise ValueError("cos_t, sin_t: [positions, head_dim / 2]")
    qa, ka, va = (np.array(t, np.float32, order="C") for t in (q, k_cache, v_cache))
    kv = int(n_kv_heads) * int(head_dim)
    if qa.size != int(n_heads) * int(head_dim) or ka.ndim != 2 or ka.shape != va.shape or ka.shape[1] != kv:
        raise ValueError("q: [n_heads * head_dim]; k_cache, v_cache: [cache_rows, n_kv_heads * head_dim]")
    ro = None if x_raw_out is None else np.array(x_raw_out, np.float32, order="C")
    if ro is not None and ro.size != kk:
        raise ValueError("x_raw_out: [k]")
    route = (C.c_int32 * 3)(-1, -1, -1)
    v = lambda t: None if t is None else t.ctypes.data_as(C.c_void_p)  # noqa: E731
    check_error(lib().kjarni_hip_op_llm_qkv_rope(device, _f(xa), None if ida is None else ida.ctypes.data_as(_ffi._u32p), v(ta),
                                                 0 if ta is None else ta.shape[0], _f(g), float(eps), v(wa), int(bool(bf16)), _f(b), kk,
                                                 int(n_heads), int(n_kv_heads), int(head_dim), _f(ca), _f(sa), ca.shape[0], int(pos),
                                                 int(bool(offset_on_device)), _f(qa), _f(ka), _f(va), ka.shape[0], _f(ro), route))
    return qa, ka, va, ro, dict(zip(("kernel", "ch", "workgroups"), list(route)))


# ---- the Whisper decoder's row projections and the front-end kernels, alone ----
(GEMV_ROWS_NOTHING, GEMV_ROWS_ONE_FAST, GEMV_ROWS_ONE_FAST_EMBED, GEMV_ROWS_STAGED_FAST, GEMV_ROWS_HEAD, GEMV_ROWS_STAGED, GEMV_ROWS_GENERAL,
 GEMV_ROWS_GEMM, GEMV_ROWS_REFUSED) = range(9)
MISALIGN_X, MISALIGN_W, MISALIGN_GAMMA, MISALIGN_BETA = 1, 2, 4, 8


def gemv_rows(x, w, rows: int, ys, k: Optional[int] = None, n_out: Optional[int] = None, gamma=None, beta=None, eps: float = 0.0, bias=None,
              r=None, r_is_y0: bool = False, seg: int = 0, row_off: int = 0, offset_on_device: bool = False, epi: int = EPI_BIAS, embed=None,
              x_raw_out=None, x_norm_out=None, misalign: int = 0, device: int = 0):
    """One launch_gemv_rows on host arrays (kjarni_hip_op_gemv_rows).  x [x_rows, ldx] (None with embed; k = w's width unless given);
    w [n_out, k]; ys: 1 or 3 outputs [out_rows, ldy] as they are before the launch (seg > 0: Q, K, V; the two caches share their
    stride); r [rows, ldr] or r_is_y0; embed: dict(id, word [vocab, k], pos_table [max_pos, k] or None, pos, pos_on_device, scale);
    x_raw_out / x_norm_out [k] as they are before the launch.  Returns (outputs, x_raw_out or None, x_norm_out or None, route) --
    copies."""
    xa = None if x is None else np.ascontiguousarray(x, np.float32)
    wa = np.ascontiguousarray(w, np.float32)
    out = [np.array(y, np.float32, order="C") for y in ys]
    if (xa is not None and xa.ndim != 2) or wa.ndim != 2 or len(out) not in (1, 3) or any(y.ndim != 2 for y in out):
        raise ValueError("x: [x_rows, ldx]; w: [n_out, k]; ys: 1 or 3 arrays [out_rows, ldy]")
    if len(out) == 3 and out[1].shape[1] != out[2].shape[1]:
        raise ValueError("ys[1] and ys[2] share ldy12")
    if (xa is None) == (embed is None):
        raise ValueError("the input row is x or the embedding: exactly one of them")
    nn = wa.shape[0] if n_out is None else int(n_out)
    kk = wa.shape[1] if k is None else int(k)
    g, be, b = _proj_vector(gamma, kk, "gamma"), _proj_vector(beta, kk, "beta"), _proj_vector(bias, max(nn, 1), "bias")
    ra = None if r is None else np.ascontiguousarray(r, np.float32)
    if ra is not None and (ra.ndim != 2 or ra.shape[0] < max(int(rows), 1)):
        raise ValueError("r: [rows, ldr]")
    raw = None if x_raw_out is None else np.array(x_raw_out, np.float32, order="C")
    nrm = None if x_norm_out is None else np.array(x_norm_out, np.float32, order="C")
    if any(t is not None and t.size != kk for t in (raw, nrm)):
        raise ValueError("x_raw_out, x_norm_out: [k]")
    ida = word = pos_t = None
    vocab = max_pos = pos = pos_dev = 0
    scale = 1.0
    if embed is not None:
        ida = np.array([int(embed["id"])], np.uint32)
        word = np.ascontiguousarray(embed["word"], np.float32)
        pos_t = None if embed.get("pos_table") is None else np.ascontiguousarray(embed["pos_table"], np.float32)
        if word.ndim != 2 or word.shape[1] != kk or (pos_t is not None and (pos_t.ndim != 2 or pos_t.shape[1] != kk)):
            raise ValueError("embed word: [vocab, k]; pos_table: [max_pos, k]")
        vocab, max_pos = word.shape[0], 0 if pos_t is None else pos_t.shape[0]
        pos, pos_dev, scale = int(embed.get("pos", 0)), int(bool(embed.get("pos_on_device", False))), float(embed.get("scale", 1.0))
    yp = (C.c_void_p * 3)(*[y.ctypes.data for y in out])
    orows = (C.c_int32 * 3)(*[y.shape[0] for y in out])
    route = C.c_int32(-1)
    check_error(lib().kjarni_hip_op_gemv_rows(device, _f(xa), 1 if xa is None else xa.shape[0], kk if xa is None else xa.shape[1], int(rows), _f(g),
                                              _f(be), float(eps), _f(wa), _f(b), _f(ra), 0 if ra is None else ra.shape[1], int(bool(r_is_y0)), nn,
                                              kk, int(seg), yp, orows, out[0].shape[1], out[1].shape[1] if len(out) == 3 else 0, int(row_off),
                                              int(bool(offset_on_device)), int(epi), None if ida is None else ida.ctypes.data_as(_ffi._u32p),
                                              _f(word), vocab, _f(pos_t), max_pos, pos, pos_dev, scale, _f(raw), _f(nrm), int(misalign),
                                              C.byref(route)))
    return out, raw, nrm, int(route.value)


def gemv_rows_route(rows: int, n_out: int, k: int, ldx: Optional[int] = None, seg: int = 0, epi: int = EPI_BIAS, gamma: bool = False,
                    beta: Optional[bool] = None, r: Optional[bool] = None, embed: bool = False, x_raw_out: bool = False, x_norm_out: bool = False,
                    misalign: int = 0) -> int:
    """gemv_rows_route (the rule launch_gemv_rows follows) for arguments given as sizes and flags; no device.  beta defaults to
    gamma, r to what the epilogue needs."""
    route = C.c_int32(-1)
    check_error(lib().kjarni_hip_gemv_rows_route(int(rows), int(n_out), int(k), int(k if ldx is None else ldx), int(seg), int(epi), int(bool(gamma)),
                                                 int(bool(gamma if beta is None else beta)), int(bool(epi == EPI_BIAS_RESIDUAL if r is None else r)),
                                                 int(bool(embed)), int(bool(x_raw_out)), int(bool(x_norm_out)), int(misalign), C.byref(route)))
    return int(route.value)


def mel_frames(audio, window, hop: int, frames, device: int = 0) -> np.ndarray:
    """launch_mel_frames on host arrays: frames [n_frames, ld] as it is before the launch; n_fft = len(window).  Returns a copy."""
    a, wn = np.ascontiguousarray(audio, np.float32).reshape(-1), np.ascontiguousarray(window, np.float32).reshape(-1)
    fr = np.array(frames, np.float32, order="C")
    if fr.ndim != 2:
        raise ValueError("frames: [n_frames, ld]")
    check_error(lib().kjarni_hip_op_mel_frames(device, _f(a), a.size, _f(wn), wn.size, int(hop), fr.shape[0], fr.shape[1], _f(fr)))
    return fr


def mel_power(dft, im_off: int, n_bins: int, power, device: int = 0) -> np.ndarray:
    """launch_mel_power: dft [n_frames, ld_dft] -> power [n_frames, ld_out] (as it is before the launch).  Returns a copy."""
    d, pw = np.ascontiguousarray(dft, np.float32), np.array(power, np.float32, order="C")
    if d.ndim != 2 or pw.ndim != 2 or d.shape[0] != pw.shape[0]:
        raise ValueError("dft: [n_frames, ld_dft]; power: [n_frames, ld_out]")
    check_error(lib().kjarni_hip_op_mel_power(device, _f(d), d.shape[1], int(im_off), int(n_bins), pw.shape[1], pw.shape[0], _f(pw)))
    return pw


def mel_log_normalize(mel, n_mels: int, out, device: int = 0):
    """launch_mel_log_normalize: mel [n_frames, ld] and out [n_frames, ld_out] as they are before the launch.  Returns copies
    (mel after the in-place log10, out)."""
    m, o = np.array(mel, np.float32, order="C"), np.array(out, np.float32, order="C")
    if m.ndim != 2 or o.ndim != 2 or m.shape[0] != o.shape[0]:
        raise ValueError("mel: [n_frames, ld]; out: [n_frames, ld_out]")
    check_error(lib().kjarni_hip_op_mel_log_normalize(device, _f(m), m.shape[1], int(n_mels), m.shape[0], o.shape[1], _f(o)))
    return m, o


def im2col3(x, channels: int, stride: int, pad: int, cols, device: int = 0) -> np.ndarray:
    """launch_im2col3: x [t_in, ldx] -> cols [t_out, ld_cols] (as it is before the launch).  Returns a copy."""
    xa, c = np.ascontiguousarray(x, np.float32), np.array(cols, np.float32, order="C")
    if xa.ndim != 2 or c.ndim != 2:
        raise ValueError("x: [t_in, ldx]; cols: [t_out, ld_cols]")
    check_error(lib().kjarni_hip_op_im2col3(device, _f(xa), xa.shape[1], xa.shape[0], int(channels), int(stride), int(pad), c.shape[0], c.shape[1],
                                            _f(c)))
    return c


def add_rows(x, period: int, table, table_rows: int, device: int = 0) -> np.ndarray:
    """launch_add_rows: x [rows, hidden] += table [r % period] where r % period < table_rows; table [>= table_rows, hidden].
    Returns a copy."""
    xa, t = np.array(x, np.float32, order="C"), np.ascontiguousarray(table, np.float32)
    if xa.ndim != 2 or t.ndim != 2 or t.shape[1] != xa.shape[1]:
        raise ValueError("x: [rows, hidden]; table: [table rows, hidden]")
    check_error(lib().kjarni_hip_op_add_rows(device, _f(xa), xa.shape[0], xa.shape[1], int(period), _f(t), int(table_rows), t.shape[0]))
    return xa


def decoder_embed(ids, word, pos, offset: int, out, offset_on_device: bool = False, scale_embeddings: bool = False, lanes: bool = False,
                  device: int = 0) -> np.ndarray:
    """launch_decoder_embed: ids [n], word [vocab, hidden], pos [max_pos, hidden] or None -> out [n, hidden] (as it is before the
    launch).  Returns a copy."""
    ia, wd = np.ascontiguousarray(ids, np.uint32).reshape(-1), np.ascontiguousarray(word, np.float32)
    pt = None if pos is None else np.ascontiguousarray(pos, np.float32)
    o = np.array(out, np.float32, order="C")
    if wd.ndim != 2 or o.shape != (ia.size, wd.shape[1]) or (pt is not None and (pt.ndim != 2 or pt.shape[1] != wd.shape[1])):
        raise ValueError("word: [vocab, hidden]; pos: [max_pos, hidden]; out: [n, hidden]")
    check_error(lib().kjarni_hip_op_decoder_embed(device, ia.ctypes.data_as(_ffi._u32p), ia.size, wd.shape[1], wd.shape[0], _f(wd), _f(pt),
                                                  0 if pt is None else pt.shape[0], int(offset), int(bool(offset_on_device)),
                                                  int(bool(scale_embeddings)), int(bool(lanes)), _f(o)))
    return o


# ---- the encoder's packed-row kernels, alone (kjarni_hip.h has the contract of every hook) ----
ATTN_NOTHING, ATTN_SPLIT, ATTN_PIPE_PADDED, ATTN_PIPE_PACKED, ATTN_PIPE_SHORT, ATTN_CHUNKED, ATTN_GENERIC = range(7)
_i32p = C.POINTER(C.c_int32)


def _u(a):
    return None if a is None else a.ctypes.data_as(_ffi._u32p)


def _i(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _cu(lengths_or_cu, is_cu):
    a = np.asarray(lengths_or_cu, np.int64).reshape(-1)
    return np.ascontiguousarray(a if is_cu else np.concatenate([[0], np.cumsum(a)]), np.int32)


def mask_lengths(mask, lens, device: int = 0) -> np.ndarray:
    """launch_mask_lengths: mask u32 [B, S] -> lens u32 [B] (as it is before the launch).  Returns a copy."""
    m, ln = np.ascontiguousarray(mask, np.uint32), np.array(lens, np.uint32, order="C")
    if m.ndim != 2 or ln.shape != (m.shape[0],):
        raise ValueError("mask: [B, S]; lens: [B]")
    check_error(lib().kjarni_hip_op_mask_lengths(device, _u(m), m.shape[0], m.shape[1], _u(ln)))
    return ln


def pack_index(mask, cu, tok_src, device: int = 0) -> np.ndarray:
    """launch_pack_index: mask u32 [B, S], cu i32 [B + 1] -> tok_src i32 [capacity] (as it is before the launch).  Returns a copy."""
    m, c, t = np.ascontiguousarray(mask, np.uint32), _cu(cu, True), np.array(tok_src, np.int32, order="C")
    if m.ndim != 2 or c.size != m.shape[0] + 1 or t.ndim != 1:
        raise ValueError("mask: [B, S]; cu: [B + 1]; tok_src: [capacity]")
    check_error(lib().kjarni_hip_op_pack_index(device, _u(m), _i(c), m.shape[0], m.shape[1], _i(t), t.size))
    return t


def encoder_embed(ids, word, out, pos=None, type=None, type_ids=None, gamma=None, beta=None, eps: float = 0.0, vocab: Optional[int] = None,
                  max_pos: Optional[int] = None, type_vocab: Optional[int] = None, pos_offset: int = 0, scale_embeddings: bool = False,
                  tok_src=None, device: int = 0) -> np.ndarray:
    """launch_embed_layernorm: ids u32 [B, S], word [>= vocab, H], pos [>= max_pos, H], type [>= type_vocab, H] -> out [rows, H] (as it
    is before the launch).  vocab / max_pos / type_vocab default to the tables' rows.  Returns a copy."""
    ia, wd, o = np.ascontiguousarray(ids, np.uint32), _c(word), np.array(out, np.float32, order="C")
    pt, tt, g, b = _c(pos), _c(type), _c(gamma), _c(beta)
    ty = None if type_ids is None else np.ascontiguousarray(type_ids, np.uint32)
    ts = None if tok_src is None else np.ascontiguousarray(tok_src, np.int32)
    if ia.ndim != 2 or wd.ndim != 2 or o.ndim != 2 or o.shape[1] != wd.shape[1] or (ts is not None and ts.shape != (o.shape[0],)) or \
            (ty is not None and ty.shape != ia.shape):
        raise ValueError("ids, type_ids: [B, S]; word: [vocab, H]; out: [rows, H]; tok_src: [rows]")
    check_error(lib().kjarni_hip_op_encoder_embed(
        device, _u(ia), _u(ty), _f(wd), _f(pt), _f(tt), _f(g), _f(b), float(eps), o.shape[0], ia.shape[0], ia.shape[1], o.shape[1],
        wd.shape[0] if vocab is None else int(vocab), (0 if pt is None else pt.shape[0]) if max_pos is None else int(max_pos),
        (0 if tt is None else tt.shape[0]) if type_vocab is None else int(type_vocab), int(pos_offset), int(bool(scale_embeddings)), _i(ts), _f(o)))
    return o


def encoder_rope(qkv, cos, sin, heads: int, head_dim: int, tok_src=None, device: int = 0) -> np.ndarray:
    """launch_rope_qk: qkv [rows, 3 * heads * head_dim] (as it is before the launch), cos / sin [S, head_dim].  Returns a copy."""
    q, c, s = np.array(qkv, np.float32, order="C"), _c(cos), _c(sin)
    ts = None if tok_src is None else np.ascontiguousarray(tok_src, np.int32)
    if q.ndim != 2 or q.shape[1] != 3 * heads * head_dim or c.shape != s.shape or c.ndim != 2 or c.shape[1] != head_dim or \
            (ts is not None and ts.shape != (q.shape[0],)):
        raise ValueError("qkv: [rows, 3 * heads * head_dim]; cos, sin: [S, head_dim]; tok_src: [rows]")
    check_error(lib().kjarni_hip_op_encoder_rope(device, _f(q), _f(c), _f(s), q.shape[0], c.shape[0], int(heads), int(head_dim), _i(ts)))
    return q


def attention_route(batch: int, seq: int, heads: int, head_dim: int, aligned: bool = True, packed: bool = False) -> Tuple[int, int]:
    """attention_route (the rule launch_attention follows): (kernel, grid of the item-per-workgroup kernels); no device."""
    r = (C.c_int32 * 2)(-1, -1)
    check_error(lib().kjarni_hip_attention_route(int(batch), int(seq), int(heads), int(head_dim), int(bool(aligned)), int(bool(packed)), r))
    return int(r[0]), int(r[1])


def attention_packed(qkv, lengths, heads: int, head_dim: int, ctx, max_len: Optional[int] = None, mask_value: float = -1e9, device: int = 0):
    """launch_attention(..., cu): qkv [buffer_rows, 3 * heads * head_dim], sentence b = rows cu[b] .. cu[b + 1] with cu the prefix
    sums of `lengths`; ctx [buffer_rows, heads * head_dim] as it is before the launch; max_len defaults to the longest sentence.
    Returns (a copy of ctx, (kernel, grid))."""
    q, o, cu = _c(qkv), np.array(ctx, np.float32, order="C"), _cu(lengths, False)
    hidden = heads * head_dim
    if q.ndim != 2 or q.shape[1] != 3 * hidden or o.shape != (q.shape[0], hidden):
        raise ValueError("qkv: [buffer_rows, 3 * hidden]; ctx: [buffer_rows, hidden]")
    r = (C.c_int32 * 2)(-1, -1)
    ml = int(np.diff(cu).max()) if max_len is None else int(max_len)
    check_error(lib().kjarni_hip_op_attention_packed(device, _f(q), _i(cu), cu.size - 1, ml, int(heads), int(head_dim), float(mask_value), _f(o),
                                                     q.shape[0], r))
    return o, (int(r[0]), int(r[1]))


def pool_packed(hidden_states, lengths, out, pooling: int = POOL_MEAN, normalize: bool = False, seq: Optional[int] = None, device: int = 0):
    """launch_pool(..., cu): hidden_states [sum(lengths), H] -> out [B, H] (as it is before the launch).  Returns a copy."""
    h, o, cu = _c(hidden_states), np.array(out, np.float32, order="C"), _cu(lengths, False)
    if h.ndim != 2 or h.shape[0] != cu[-1] or o.shape != (cu.size - 1, h.shape[1]):
        raise ValueError("hidden_states: [sum(lengths), H]; out: [B, H]")
    check_error(lib().kjarni_hip_op_pool_packed(device, _f(h), _i(cu), cu.size - 1, int(np.diff(cu).max()) if seq is None else int(seq), h.shape[1],
                                                int(pooling), int(bool(normalize)), _f(o)))
    return o


def small_linear(feat, w, bias, out, k: Optional[int] = None, device: int = 0) -> np.ndarray:
    """launch_small_linear: feat [rows, ld] (the first k columns of every row), w [n, k], bias [n] or None -> out [rows, n] (as it is
    before the launch).  Returns a copy."""
    x, wt, b, o = _c(feat), _c(w), _c(bias), np.array(out, np.float32, order="C")
    if x.ndim != 2 or wt.ndim != 2 or o.shape != (x.shape[0], wt.shape[0]):
        raise ValueError("feat: [rows, ld]; w: [n, k]; out: [rows, n]")
    check_error(lib().kjarni_hip_op_small_linear(device, _f(x), x.shape[1], _f(wt), _f(b), x.shape[0], wt.shape[1] if k is None else int(k),
                                                 wt.shape[0], _f(o)))
    return o


def row_softmax(x, out, sigmoid: bool = False, device: int = 0) -> np.ndarray:
    """launch_row_softmax: x [rows, n] -> out [rows, n] (as it is before the launch).  Returns a copy."""
    a, o = _c(x), np.array(out, np.float32, order="C")
    if a.ndim != 2 or o.shape != a.shape:
        raise ValueError("x, out: [rows, n]")
    check_error(lib().kjarni_hip_op_row_softmax(device, _f(a), a.shape[0], a.shape[1], int(bool(sigmoid)), _f(o)))
    return o


# ---- mixture-of-experts: the router pick and the sparse FFN, alone ----
def moe_route(logits, k: int, norm_topk: bool = False, device: int = 0):
    """launch_moe_route on host arrays (kjarni_hip_op_moe_route): logits [rows, E] -> (ids int32 [rows, k], weights f32 [rows, k]),
    slot 0 the largest, the lower expert first on equal logits."""
    la = np.ascontiguousarray(logits, np.float32)
    if la.ndim != 2:
        raise ValueError("logits: [rows, E]")
    rows, e = la.shape
    ids = np.full((rows, max(int(k), 0)), -1, np.int32)
    w = np.full((rows, max(int(k), 0)), np.nan, np.float32)
    check_error(lib().kjarni_hip_op_moe_route(device, _f(la), rows, e, int(k), int(bool(norm_topk)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                              _f(w)))
    return ids, w


def moe_ffn(x, router, gate, up, down, k: int, y, r=None, r_is_y: bool = False, gamma=None, eps: float = 1e-6, norm_topk: bool = False,
            bf16: bool = False, route: int = 0, hidden: Optional[int] = None, device: int = 0):
    """The sparse FFN on host arrays (kjarni_hip_op_moe_ffn): x [rows, ldx]; router [E, hidden], gate / up [E, Im, hidden], down
    [E, hidden, Im] f32 or bf16 bit patterns (uint16, bf16 = True); y [rows, ldy] given with whatever its padding holds; r [rows, ldr]
    or r_is_y.  route: 0 the decoders' rule, 1 steps, 2 grouped.  Returns (y, ids, weights, route_used, tiles_used) -- copies."""
    wt = np.uint16 if bf16 else np.float32
    xa = np.ascontiguousarray(x, np.float32)
    ra_, ga, ua, da = (np.ascontiguousarray(t, wt) for t in (router, gate, up, down))
    ya = np.array(y, np.float32, order="C")
    if xa.ndim != 2 or ya.ndim != 2 or ya.shape[0] != xa.shape[0] or ra_.ndim != 2 or ga.ndim != 3 or ua.shape != ga.shape or da.ndim != 3:
        raise ValueError("x: [rows, ldx]; y: [rows, ldy]; router: [E, hidden]; gate, up: [E, Im, hidden]; down: [E, hidden, Im]")
    e, im, h = ga.shape
    if ra_.shape != (e, h) or da.shape != (e, h, im) or (hidden is not None and int(hidden) != h):
        raise ValueError("router: [E, hidden]; down: [E, hidden, Im]")
    rows = xa.shape[0]
    gm = _proj_vector(gamma, h, "gamma")
    rr = None if r is None else np.ascontiguousarray(r, np.float32)
    if rr is not None and (rr.ndim != 2 or rr.shape[0] != rows):
        raise ValueError("r: [rows, ldr]")
    kk = max(int(k), 0)
    ids, w = np.full((rows, kk), -1, np.int32), np.full((rows, kk), np.nan, np.float32)
    used, tiles = C.c_int32(-1), C.c_int32(-1)
    v = lambda t: t.ctypes.data_as(C.c_void_p)  # noqa: E731
    check_error(lib().kjarni_hip_op_moe_ffn(device, _f(xa), xa.shape[1], rows, _f(gm), float(eps), v(ra_), v(ga), v(ua), v(da), int(bool(bf16)), h, e,
                                            int(k), im, int(bool(norm_topk)), _f(rr), 0 if rr is None else rr.shape[1], int(bool(r_is_y)), _f(ya),
                                            ya.shape[1], int(route), ids.ctypes.data_as(C.POINTER(C.c_int32)), _f(w), C.byref(used),
                                            C.byref(tiles)))
    return ya, ids, w, used.value, tiles.value


def prefill_attention(q, k, v, ldk: int, ldv: int, base: int, heads: int, head_dim: int, kv_group: int = 1, ctx=None, device: int = 0):
    """launch_prefill_attention on host arrays (kjarni_hip_op_prefill_attention): q [rows, ldq]; k and v flat float buffers, key row
    t at t * ldk; row s sees keys <= base + s.  Returns (ctx [rows, ldc] -- given, or NaN [rows, heads * head_dim] -- with the context
    rows written, route): 0 the vector kernel, 1 the matrix-core kernel."""
    qa = np.ascontiguousarray(q, np.float32)
    ka, va = np.ascontiguousarray(k, np.float32).reshape(-1), np.ascontiguousarray(v, np.float32).reshape(-1)
    if qa.ndim != 2:
        raise ValueError("q: [rows, ldq]")
    rows = qa.shape[0]
    ca = np.full((rows, heads * head_dim), np.nan, np.float32) if ctx is None else np.array(ctx, np.float32, order="C")
    if ca.ndim != 2 or ca.shape[0] != rows:
        raise ValueError("ctx: [rows, ldc]")
    route = C.c_int32(-1)
    check_error(lib().kjarni_hip_op_prefill_attention(device, _f(qa), qa.shape[1], rows, _f(ka), ka.size, int(ldk), _f(va), va.size, int(ldv),
                                                      int(base), int(heads), int(head_dim), int(kv_group), _f(ca), ca.shape[1], C.byref(route)))
    return ca, route.value


# ---- the decode step's fused projections and their preparation kernels, alone ----
PROJ_PLAIN, PROJ_QKV, PROJ_SWIGLU = 0, 1, 2


def _proj_common(mats, x, ys, r, rows, in_place=False):
    """The arrays both fused-projection entries take: x [rows_alloc, ldx], ys copied (the entry writes into the copies; in_place:
    into ys themselves, which must then be C-contiguous float32 arrays -- a refused call must leave them as they are)."""
    xa = np.ascontiguousarray(x, np.float32)
    if in_place and any(not (isinstance(y, np.ndarray) and y.dtype == np.float32 and y.flags.c_contiguous) for y in ys):
        raise ValueError("in_place: ys must be C-contiguous float32 arrays")
    out = list(ys) if in_place else [np.array(y, np.float32, order="C") for y in ys]
    if xa.ndim != 2 or any(y.ndim != 2 for y in out) or not 1 <= len(out) <= 3 or not 1 <= len(mats) <= 3:
        raise ValueError("x: [rows_alloc, ldx]; ys: 1-3 arrays [out_rows, ldy]; 1-3 matrices")
    yp = (C.c_void_p * 3)(*[y.ctypes.data for y in out])
    orows = (C.c_int32 * 3)(*[y.shape[0] for y in out])
    ldy = (C.c_int64 * 3)(*[y.shape[1] for y in out])
    ra = None if r is None else np.ascontiguousarray(r, np.float32)
    if ra is not None and (ra.ndim != 2 or ra.shape[0] < max(int(rows), 1)):
        raise ValueError("r: [rows, ldr]")
    return xa, out, yp, orows, ldy, ra


def _proj_vector(a, n, what):
    """A vector the entry reads n floats of."""
    a = _c(a)
    if a is not None and a.size != n:
        raise ValueError(f"{what}: {n} floats, not {a.size}")
    return a


_GGML_BLOCK = {8: (32, 34), 12: (256, 144), 14: (256, 210)}      # type: (elements, bytes) per block


def _ggml_blocks(ggml_type, blocks, n, k):
    """Raw blocks [n, bytes per row] of a type this module knows, checked against k (the entry refuses the other types, and a k
    that is no whole number of blocks, before it reads them)."""
    ba = np.ascontiguousarray(blocks, np.uint8)
    be, bb = _GGML_BLOCK.get(int(ggml_type), (0, 0))
    if be and k % be == 0 and ba.size != n * (k // be) * bb:
        raise ValueError(f"blocks: {n} rows of {k // be} blocks of {bb} bytes, not {ba.size} bytes")
    return ba


def fused_proj_fp8(mode: int, mats, x, rows: int, ys, gamma=None, eps: float = 0.0, bias=None, r=None, r_is_y0: bool = False,
                   row_off: int = 0, offset_on_device: bool = False, in_place: bool = False, device: int = 0):
    """One launch_fp8_proj on host arrays (kjarni_hip_op_fused_proj_fp8).  mats: 1-3 of (codes uint8 [n, k], scale f32
    [scale_rows, scale_cols]); x [rows_alloc, ldx]; ys: the mode's outputs [out_rows, ldy] as they are before the launch.  Returns
    the outputs after it."""
    xa, out, yp, orows, ldy, ra = _proj_common(mats, x, ys, r, rows, in_place)
    codes = [np.ascontiguousarray(c, np.uint8) for c, _ in mats]
    scales = [np.ascontiguousarray(s, np.float32) for _, s in mats]
    if any(c.ndim != 2 or s.ndim != 2 for c, s in zip(codes, scales)):
        raise ValueError("codes [n, k], scale [scale_rows, scale_cols]")
    cp = (C.c_void_p * 3)(*[c.ctypes.data for c in codes])
    sp = (C.c_void_p * 3)(*[s.ctypes.data for s in scales])
    sr = (C.c_int32 * 3)(*[s.shape[0] for s in scales])
    sc = (C.c_int32 * 3)(*[s.shape[1] for s in scales])
    n = (C.c_int32 * 3)(*[c.shape[0] for c in codes])
    k = codes[0].shape[1]
    if any(c.shape[1] != k for c in codes):
        raise ValueError("the matrices must share k")
    g = _proj_vector(gamma, k, "gamma")
    b = _proj_vector(bias, codes[0].shape[0] if int(mode) != PROJ_QKV else sum(c.shape[0] for c in codes), "bias (the concatenated columns)")
    check_error(lib().kjarni_hip_op_fused_proj_fp8(device, int(mode), cp, sp, sr, sc, n, k, _f(xa), xa.shape[0], xa.shape[1],
                                                   int(rows), _f(g), float(eps), _f(b), _f(ra), 0 if ra is None else ra.shape[1],
                                                   int(bool(r_is_y0)), yp, orows, ldy, int(row_off), int(bool(offset_on_device))))
    return out


def fused_proj_ggml(mode: int, mats, x, rows: int, ys, gamma=None, eps: float = 0.0, bias=None, bias_off=(0, 0, 0), r=None,
                    r_is_y0: bool = False, row_off: int = 0, offset_on_device: bool = False, head_dim: int = 0, cos=None, sin=None,
                    q8k: bool = False, k: Optional[int] = None, in_place: bool = False, device: int = 0):
    """One launch_qfused on host arrays (kjarni_hip_op_fused_proj_ggml), after launch_qprep when q8k.  mats: 1-3 of (ggml type, raw
    blocks uint8 [n, bytes per row]); k: the matrices' columns (default: x's).  Returns (outputs, None), or with q8k (outputs,
    (xn [rows, k] -- NaN without gamma --, codes int8 [rows, k], scales [rows, k // 256])) as the device produced them."""
    xa, out, yp, orows, ldy, ra = _proj_common(mats, x, ys, r, rows, in_place)
    k = xa.shape[1] if k is None else int(k)
    if any(np.ndim(b) != 2 for _, b in mats):
        raise ValueError("blocks [n, bytes per row]")
    blocks = [_ggml_blocks(t, b, np.shape(b)[0], k) for t, b in mats]
    bp = (C.c_void_p * 3)(*[b.ctypes.data for b in blocks])
    ty = (C.c_int32 * 3)(*[int(t) for t, _ in mats])
    n = (C.c_int32 * 3)(*[b.shape[0] for b in blocks])
    g, b = _proj_vector(gamma, k, "gamma"), _c(bias)      # (the entry holds bias_off + n against the bias's own length)
    boff = (C.c_int32 * 3)(*[int(v) for v in bias_off])
    ct = st = None
    if cos is not None:
        ct, st = _tables(cos, sin, head_dim)
    rws = max(int(rows), 1)
    xn = np.full((rws, k), np.nan, np.float32)
    xq = np.zeros((rws, k), np.int8)
    xd = np.full((rws, max(k // 256, 1)), np.nan, np.float32)
    check_error(lib().kjarni_hip_op_fused_proj_ggml(device, int(mode), bp, ty, n, k, _f(xa), xa.shape[0], xa.shape[1], int(rows), _f(g), float(eps),
                                                    _f(b), 0 if b is None else b.size, boff, _f(ra), 0 if ra is None else ra.shape[1],
                                                    int(bool(r_is_y0)), yp, orows, ldy, int(row_off), int(bool(offset_on_device)), int(head_dim),
                                                    _f(ct), _f(st), 0 if ct is None else ct.shape[0], int(bool(q8k)), _f(xn),
                                                    xq.ctypes.data_as(C.c_void_p), _f(xd)))
    return out, ((xn, xq, xd) if q8k else None)


def qembed(ids, ggml_type: int, blocks, vocab: int, k: int, out=None, device: int = 0):
    """launch_qembed alone (kjarni_hip_op_qembed): the dequantized table rows ids[i] [len(ids), k]; an id >= vocab gives zeros."""
    ia = np.ascontiguousarray(ids, np.uint32)
    ba = _ggml_blocks(ggml_type, blocks, int(vocab), int(k))
    oa = np.full((ia.size, k), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
    if oa.size != ia.size * k:
        raise ValueError("out: [len(ids), k]")
    check_error(lib().kjarni_hip_op_qembed(device, ia.ctypes.data_as(C.POINTER(C.c_uint32)), ia.size, ba.ctypes.data_as(C.c_void_p),
                                           int(ggml_type), int(vocab), int(k), _f(oa)))
    return oa


def q8k_quantize(x, k: int, device: int = 0):
    """launch_q8k_quantize alone (kjarni_hip_op_q8k_quantize): x [rows, ldx] -> (codes int8 [rows, k], scales [rows, k // 256],
    deq [rows, k])."""
    xa = np.ascontiguousarray(x, np.float32)
    rows = xa.shape[0]
    codes, scales, deq = np.zeros((rows, k), np.int8), np.full((rows, max(k // 256, 1)), np.nan, np.float32), np.full((rows, k), np.nan, np.float32)
    check_error(lib().kjarni_hip_op_q8k_quantize(device, _f(xa), rows, xa.shape[1], int(k), codes.ctypes.data_as(C.c_void_p), _f(scales), _f(deq)))
    return codes, scales, deq


def _tables(cos, sin, head_dim):
    ct, st = np.ascontiguousarray(cos, np.float32), np.ascontiguousarray(sin, np.float32)
    if ct.ndim != 2 or ct.shape != st.shape or ct.shape[1] != head_dim // 2:
        raise ValueError("cos and sin: [table_rows, head_dim // 2]")
    return ct, st


def rope(x, rows: int, n_heads: int, head_dim: int, cos, sin, pos: int, device: int = 0):
    """The RoPE kernel of the prompt and decode paths alone: x [x_rows, ldx] -> x with its first `rows` rows rotated by table
    rows pos, pos + 1, ..."""
    xa = np.array(x, np.float32, order="C")
    ct, st = _tables(cos, sin, head_dim)
    check_error(lib().kjarni_hip_op_rope(device, _f(xa), xa.shape[1], xa.shape[0], int(rows), int(n_heads), int(head_dim), _f(ct), _f(st),
                                         ct.shape[0], int(pos)))
    return xa


def rope_rows(x, row_pos, n_heads: int, head_dim: int, cos, sin, device: int = 0):
    """rope() with row r rotated by table row row_pos[r]; len(row_pos) rows are processed."""
    xa = np.array(x, np.float32, order="C")
    rp = np.ascontiguousarray(row_pos, np.int32)
    ct, st = _tables(cos, sin, head_dim)
    check_error(lib().kjarni_hip_op_rope_rows(device, _f(xa), xa.shape[1], xa.shape[0], rp.size, int(n_heads), int(head_dim), _f(ct), _f(st),
                                              ct.shape[0], rp.ctypes.data_as(_i32p)))
    return xa


def qk_norm_rope_rows(q, k, row_pos, n_heads: int, n_kv_heads: int, head_dim: int, gamma_q, gamma_k, eps: float, cos, sin, device: int = 0):
    """qk_norm_rope() with row r at position row_pos[r] (its K heads are row r of k): (q, k) after the call on len(row_pos)
    rows."""
    qa, ka = np.array(q, np.float32, order="C"), np.array(k, np.float32, order="C")
    gq, gk = np.ascontiguousarray(gamma_q, np.float32), np.ascontiguousarray(gamma_k, np.float32)
    rp = np.ascontiguousarray(row_pos, np.int32)
    ct, st = _tables(cos, sin, head_dim)
    if qa.ndim != 2 or ka.ndim != 2 or gq.shape != (head_dim,) or gk.shape != (head_dim,):
        raise ValueError("q and k: [rows, ld]; gammas: [head_dim]")
    check_error(lib().kjarni_hip_op_qk_norm_rope_rows(device, _f(qa), qa.shape[1], qa.shape[0], _f(ka), ka.shape[1], ka.shape[0], rp.size,
                                                      int(n_heads), int(n_kv_heads), int(head_dim), _f(gq), _f(gk), float(eps), _f(ct), _f(st),
                                                      ct.shape[0], rp.ctypes.data_as(_i32p)))
    return qa, ka


def last_token_pool(x, lengths, gamma, eps: float, normalize: bool = True, hidden=None, device: int = 0):
    """The last-token pool alone: x [rows, ldx] holds the sequences of `lengths` one after another; returns
    [len(lengths), hidden] -- every sequence's last row through RMSNorm(gamma, eps) and, when `normalize`, divided by its L2 norm
    where that is > 0."""
    xa = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    hidden = g.size if hidden is None else int(hidden)
    st = _seq_start(lengths)
    out = np.zeros((st.size - 1, hidden), np.float32)
    check_error(lib().kjarni_hip_op_last_token_pool(device, _f(xa), xa.shape[1], xa.shape[0], st.ctypes.data_as(_i32p), st.size - 1, hidden,
                                                    _f(g), float(eps), int(bool(normalize)), _f(out)))
    return out


def packed_prefix_attention(q, k, v, remainders, heads: int, kv_heads: int, head_dim: int, ctx=None, device: int = 0):
    """The prefix attention kernel of HipDecoder.score_batch alone: q / k / v / ctx as packed_causal_attention takes them;
    remainders: rows of (first row, rows, the prefix's first row, prefix rows).  Row t of a remainder attends to its prefix rows
    and to the remainder's rows 0 .. t.  Returns ctx with the remainders' context rows written; everything else as it was."""
    qa, ka, va = (np.ascontiguousarray(x, np.float32) for x in (q, k, v))
    ca = np.zeros((qa.shape[0], heads * head_dim), np.float32) if ctx is None else np.array(ctx, np.float32, order="C")
    if any(x.ndim != 2 or x.shape[0] != qa.shape[0] for x in (qa, ka, va, ca)):
        raise ValueError("q, k, v, ctx: [rows, ld] with the same rows")
    rem = np.ascontiguousarray(remainders, np.int32).reshape(-1, 4)
    check_error(lib().kjarni_hip_op_packed_prefix_attention(device, _f(qa), qa.shape[1], _f(ka), ka.shape[1], _f(va), va.shape[1], qa.shape[0],
                                                            rem.ctypes.data_as(_i32p), rem.shape[0], int(heads), int(kv_heads), int(head_dim),
                                                            _f(ca), ca.shape[1]))
    return ca


def score_gather_norm(x, src, gamma, beta=None, eps: float = 1e-5, hidden=None, out=None, device: int = 0):
    """The gather + final norm of HipDecoder.score_batch alone: out[j, :hidden] = norm(x[src[j], :hidden]) -- RMSNorm(gamma, eps),
    or LayerNorm(gamma, beta, eps) when beta is given.  out: given ([len(src), ldo], its other columns come back as they were), or
    zeros [len(src), hidden]."""
    xa = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    b = None if beta is None else np.ascontiguousarray(beta, np.float32)
    hidden = g.size if hidden is None else int(hidden)
    s = np.ascontiguousarray(src, np.int32)
    oa = np.zeros((s.size, hidden), np.float32) if out is None else np.array(out, np.float32, order="C")
    if xa.ndim != 2 or oa.ndim != 2 or oa.shape[0] != s.size:
        raise ValueError("x: [rows, ldx]; out: [len(src), ldo]")
    check_error(lib().kjarni_hip_op_score_gather_norm(device, _f(xa), xa.shape[1], xa.shape[0], s.ctypes.data_as(_i32p), s.size, hidden, _f(g),
                                                      _f(b) if b is not None else None, float(eps), _f(oa), oa.shape[1]))
    return oa


def answer_logits(x, src, gamma, head, targets, beta=None, eps: float = 1e-6, hidden=None, head_is_bf16: bool = False, device: int = 0):
    """The answer-logits kernel of HipDecoder.answer_logits alone: out[j, t] = dot(norm(x[src[j], :hidden]), head[targets[t], :]) --
    RMSNorm(gamma, eps), or LayerNorm(gamma, beta, eps) when beta is given.  x: [rows, ldx] f32; head: [head_rows, hidden] f32, or
    uint16 bf16 bit patterns with head_is_bf16.  Returns f32 [len(src), len(targets)]."""
    xa = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    b = None if beta is None else np.ascontiguousarray(beta, np.float32)
    hidden = g.size if hidden is None else int(hidden)
    ha = np.ascontiguousarray(head, np.uint16 if head_is_bf16 else np.float32)
    s, t = np.ascontiguousarray(src, np.int32), np.ascontiguousarray(targets, np.uint32)
    if xa.ndim != 2 or ha.ndim != 2 or ha.shape[1] != hidden:
        raise ValueError("x: [rows, ldx]; head: [head_rows, hidden]")
    out = np.zeros(max(s.size * t.size, 1), np.float32)
    tp = t if t.size else np.zeros(1, np.uint32)        # (an empty list still reaches the check that names n_targets)
    check_error(lib().kjarni_hip_op_answer_logits(device, _f(xa), xa.shape[1], xa.shape[0], s.ctypes.data_as(_i32p), s.size, hidden, _f(g),
                                                  _f(b) if b is not None else None, float(eps), ha.ctypes.data_as(C.c_void_p), ha.shape[0],
                                                  int(bool(head_is_bf16)), tp.ctypes.data_as(_ffi._u32p), t.size, _f(out)))
    return out[:s.size * t.size].reshape(s.size, t.size)


def answer_plan(seqs, head_dim: int = 64, min_shared: Optional[int] = None) -> dict:
    """The plan of HipDecoder.answer_logits (no GPU): decoder.answer_plan."""
    from . import decoder
    return decoder.answer_plan(seqs, head_dim, decoder.SCORE_MIN_SHARED if min_shared is None else min_shared)


def argmax(logits, vocab: Optional[int] = None, route: int = ARGMAX_DECODER, live=None, draft=None, device: int = 0):
    """The greedy pick kernels on logits [calls, rows, ld] (the last of equal maxima wins; columns >= vocab are padding).
    Returns picks int32 [calls, rows]: decoder route rows == 1; lanes route -1 for the lanes `live` [rows] freezes; lookup
    route (picks, accepted) with draft [calls, n_draft], picks[c, :accepted[c] + 1] the verify step's tokens, -1 past them."""
    lg = np.ascontiguousarray(logits, np.float32)
    calls, rows, ld = lg.shape
    vocab = ld if vocab is None else int(vocab)
    picks = np.full((calls, rows), -2, np.int32)
    acc = np.zeros(calls, np.int32)
    lv = None if live is None else np.ascontiguousarray(live, np.int32)
    dr = None if draft is None else np.ascontiguousarray(draft, np.uint32).reshape(calls, -1)
    if lv is not None and lv.size != rows:
        raise ValueError("live must hold one flag per row")
    n_draft = 0 if dr is None else dr.shape[1]
    check_error(lib().kjarni_hip_op_argmax(device, _f(lg), calls, rows, ld, vocab, route, None if lv is None else lv.ctypes.data_as(_i32p),
                                           None if dr is None else dr.ctypes.data_as(_ffi._u32p), n_draft, picks.ctypes.data_as(_i32p),
                                           acc.ctypes.data_as(_i32p)))
    return (picks, acc) if route == ARGMAX_LOOKUP else picks


def token_logprob_slabs(rows: int, vocab: int) -> int:
    """The slabs the generation log-probability kernels cut a row of `vocab` logits into when `rows` rows run together (no GPU)."""
    return int(lib().kjarni_hip_token_logprob_slabs(int(rows), int(vocab)))


def token_logprobs(logits, tokens, top_k: int, vocab: Optional[int] = None, device: int = 0, out=None):
    """The generation log-probability kernels on logits [calls, rows, ld] (columns >= vocab are padding) and the chosen tokens
    [calls, rows] (-1: the row is skipped and its outputs come back as `out` gave them).  Returns a dict: logprob, lse
    [calls, rows], topk_ids, topk_logprob [calls, rows, top_k], slabs.  out: (logprob, topk_ids, topk_logprob, lse) initial values
    (default NaN / 0xFFFFFFFF)."""
    lg = np.ascontiguousarray(logits, np.float32)
    calls, rows, ld = lg.shape
    vocab = ld if vocab is None else int(vocab)
    tk = np.ascontiguousarray(tokens, np.int32).reshape(calls, rows)
    k = max(int(top_k), 0)
    if out is None:
        lp, lse = np.full((calls, rows), np.nan, np.float32), np.full((calls, rows), np.nan, np.float32)
        ids, tlp = np.full((calls, rows, k), 0xFFFFFFFF, np.uint32), np.full((calls, rows, k), np.nan, np.float32)
    else:
        lp, ids, tlp, lse = (np.ascontiguousarray(a).copy() for a in out)
    slabs = C.c_int32(0)
    check_error(lib().kjarni_hip_op_token_logprobs(device, _f(lg), calls, rows, ld, vocab, tk.ctypes.data_as(_i32p), int(top_k), _f(lp),
                                                   ids.ctypes.data_as(_ffi._u32p) if ids.size else None, _f(tlp) if tlp.size else None,
                                                   _f(lse), C.byref(slabs)))
    return {"logprob": lp, "topk_ids": ids, "topk_logprob": tlp, "lse": lse, "slabs": int(slabs.value)}


def token_logprobs_bench(logits, top_k: int = 8, iters: int = 50, device: int = 0):
    """(pair ms, score-rows ms) per pass over logits [rows, vocab]: the generation log-probability launch pair, and the
    one-workgroup-per-row score kernel over the same rows 8 at a time (tools/bench_more.py llm_logprobs)."""
    lg = np.ascontiguousarray(logits, np.float32)
    rows, vocab = lg.shape
    a, b = C.c_float(0), C.c_float(0)
    check_error(lib().kjarni_hip_op_token_logprobs_bench(device, _f(lg), rows, vocab, int(top_k), int(iters), C.byref(a), C.byref(b)))
    return float(a.value), float(b.value)


def whisper_pick(logits, first_special: int, eos: int, timestamp_begin: int, allow_timestamps: bool, two_launch: bool, device: int = 0):
    """Whisper's pick on logits [calls, lanes, vocab]: tokens int32 [calls, lanes]; two_launch chooses the replayed step's
    two small launches over the one 1024-thread workgroup per lane."""
    lg = np.ascontiguousarray(logits, np.float32)
    calls, lanes, vocab = lg.shape
    out = np.full((calls, lanes), -2, np.int32)
    check_error(lib().kjarni_hip_op_whisper_pick(device, _f(lg), calls, lanes, vocab, first_special, eos, timestamp_begin, int(allow_timestamps),
                                                 int(two_launch), out.ctypes.data_as(_i32p)))
    return out


def logits_processors(logits, tokens, n_bulk: int, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0, device: int = 0):
    """Repetition penalty + n-gram ban of the history `tokens` on the device; the per-token counts come from one launch over
    tokens[:n_bulk] and one launch per later token, as in a generate call."""
    lg = np.ascontiguousarray(logits, np.float32)
    t = np.ascontiguousarray(tokens, np.uint32)
    out = np.empty_like(lg)
    check_error(lib().kjarni_hip_op_logits_processors(device, _f(lg), lg.size, t.ctypes.data_as(_ffi._u32p), t.size, n_bulk,
                                                      repetition_penalty, no_repeat_ngram, _f(out)))
    return out


def constraint_mask(trans, tok_off, tok_bytes, device: int = 0):
    """The constrained-decoding mask build alone: trans uint16 [S, 256], the token table (tok_off [V + 1], tok_bytes).  Returns
    (mask uint64 [S, ceil(V / 64)], counts uint32 [S])."""
    tr = np.ascontiguousarray(trans, np.uint16)
    off = np.ascontiguousarray(tok_off, np.uint32)
    by = np.ascontiguousarray(tok_bytes, np.uint8)
    S, V = tr.shape[0], off.size - 1
    mask = np.empty((S, (V + 63) // 64), np.uint64)
    counts = np.empty(S, np.uint32)
    check_error(lib().kjarni_hip_op_constraint_mask(device, tr.ctypes.data_as(C.POINTER(C.c_uint16)), S, off.ctypes.data_as(_ffi._u32p),
                                                    by.ctypes.data_as(C.POINTER(C.c_uint8)) if by.size else None, V,
                                                    mask.ctypes.data_as(C.POINTER(C.c_uint64)), counts.ctypes.data_as(_ffi._u32p)))
    return mask, counts


def constraint_apply(constraint, logits, states, done, stop_ids=(), device: int = 0):
    """The mask applied to logits [rows, ld] (ld >= the constraint's vocabulary) with a state and a done flag per row: the
    whole buffer back, the columns past the vocabulary included."""
    lg = np.ascontiguousarray(logits, np.float32)
    rows, ld = lg.shape
    st = np.ascontiguousarray(states, np.uint32)
    dn = np.ascontiguousarray(done, np.int32)
    sp = np.ascontiguousarray(stop_ids, np.uint32)
    if st.size != rows or dn.size != rows:
        raise ValueError("one state and one done flag per row")
    out = np.empty_like(lg)
    check_error(lib().kjarni_hip_op_constraint_apply(device, constraint._h, _f(lg), rows, ld, st.ctypes.data_as(_ffi._u32p),
                                                     dn.ctypes.data_as(_i32p), sp.ctypes.data_as(_ffi._u32p) if sp.size else None, sp.size,
                                                     _f(out)))
    return out


def constraint_advance(constraint, picked, states, done, stop_ids=(), device: int = 0):
    """The automaton step alone: (states, done, violated) after the picks, one per row."""
    pk = np.ascontiguousarray(picked, np.int32)
    st = np.array(states, np.uint32)
    dn = np.array(done, np.int32)
    sp = np.ascontiguousarray(stop_ids, np.uint32)
    if st.size != pk.size or dn.size != pk.size:
        raise ValueError("one state and one done flag per pick")
    bad = np.full(pk.size, -2, np.int32)
    check_error(lib().kjarni_hip_op_constraint_advance(device, constraint._h, pk.ctypes.data_as(_i32p), pk.size, st.ctypes.data_as(_ffi._u32p),
                                                       dn.ctypes.data_as(_i32p), sp.ctypes.data_as(_ffi._u32p) if sp.size else None, sp.size,
                                                       bad.ctypes.data_as(_i32p)))
    return st, dn, bad


def sample_candidates(rows, top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                      capacity: int = 4096, device: int = 0):
    """The sampler's device cut over each of `rows` (1-D logits arrays, possibly of different lengths), in order, on one
    scratch / header / candidate buffer.  Per row a dict: mx, sum, floor (np.float32), count, overflow, ids (uint32) and
    logits (float32) of the first min(count, capacity) candidates."""
    rows = [np.ascontiguousarray(r, np.float32).ravel() for r in rows]
    flat = np.concatenate(rows)
    vocabs = np.array([r.size for r in rows], np.int32)
    hdr = (_ffi.KjarniHipSampleHeader * len(rows))()
    ids = np.zeros((len(rows), capacity), np.uint32)
    vals = np.zeros((len(rows), capacity), np.float32)
    check_error(lib().kjarni_hip_op_sample_candidates(device, _f(flat), vocabs.ctypes.data_as(_i32p), len(rows), -1 if top_k is None else top_k,
                                                      -1.0 if top_p is None else top_p, -1.0 if min_p is None else min_p, capacity, hdr,
                                                      ids.ctypes.data_as(_ffi._u32p), _f(vals)))
    out = []
    for c, h in enumerate(hdr):
        n = min(int(h.count), capacity)
        out.append({"mx": np.float32(h.mx), "sum": np.float32(h.sum), "floor": np.float32(h.floor), "count": int(h.count),
                    "overflow": int(h.overflow), "ids": ids[c, :n].copy(), "logits": vals[c, :n].copy()})
    return out


def sample_candidates_rows(block, vocab: Optional[int] = None, top_k: Optional[int] = None, top_p: Optional[float] = None,
                           min_p: Optional[float] = None, capacity: int = 4096, device: int = 0):
    """The sampler's cut over the rows of `block` ([rows, ld] logits, rows 1..8, the first `vocab` columns of every row) in one
    chain of three launches.  Per row a dict as sample_candidates() gives, plus "slots": every one of the row's `capacity`
    (id, logit-bits) slots as uint32 [capacity, 2] (0xffffffff where nothing was written)."""
    lg = np.ascontiguousarray(block, np.float32)
    rows, ld = lg.shape
    vocab = ld if vocab is None else int(vocab)
    hdr = (_ffi.KjarniHipSampleHeader * rows)()
    ids = np.zeros((rows, capacity), np.uint32)
    vals = np.zeros((rows, capacity), np.float32)
    check_error(lib().kjarni_hip_op_sample_candidates_rows(device, _f(lg), ld, rows, vocab, -1 if top_k is None else top_k,
                                                           -1.0 if top_p is None else top_p, -1.0 if min_p is None else min_p, capacity, hdr,
                                                           ids.ctypes.data_as(_ffi._u32p), _f(vals)))
    out = []
    for c, h in enumerate(hdr):
        n = 0 if h.floor == -np.inf else min(int(h.count), capacity)
        out.append({"mx": np.float32(h.mx), "sum": np.float32(h.sum), "floor": np.float32(h.floor), "count": int(h.count),
                    "overflow": int(h.overflow), "ids": ids[c, :n].copy(), "logits": vals[c, :n].copy(),
                    "slots": np.stack([ids[c], vals[c].view(np.uint32)], axis=1)})
    return out


def repetition_penalty_rows(block, ids, history, penalty: float, vocab: Optional[int] = None, device: int = 0):
    """The repetition penalty over the rows of a verify block on the device: block [rows, ld]; `history` ends with ids[0]; row
    r is penalised for history + ids[1:r + 1].  Returns the processed block."""
    lg = np.ascontiguousarray(block, np.float32)
    rows, ld = lg.shape
    vocab = ld if vocab is None else int(vocab)
    i = np.ascontiguousarray(ids, np.uint32)
    h = np.ascontiguousarray(history, np.uint32)
    if i.size < rows:
        raise ValueError("ids needs one entry per row")
    out = np.empty_like(lg)
    check_error(lib().kjarni_hip_op_repetition_penalty_rows(device, _f(lg), ld, rows, vocab, i.ctypes.data_as(_ffi._u32p),
                                                            h.ctypes.data_as(_ffi._u32p) if h.size else None, h.size, penalty, _f(out)))
    return out


def lookup_accept_sampled(block, draft, uniforms, temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                          min_p: Optional[float] = None, vocab: Optional[int] = None):
    """Deciding a verify block on the host (no GPU): block [rows, ld] processed logits, the draft, one draw per decided row.
    Returns (picks, accepted, draws_used)."""
    lg = np.ascontiguousarray(block, np.float32)
    rows, ld = lg.shape
    vocab = ld if vocab is None else int(vocab)
    d = np.ascontiguousarray(draft, np.uint32)
    u = np.ascontiguousarray(uniforms, np.float32)
    if u.size < min(d.size, rows - 1) + 1:
        raise ValueError("one draw per row that may be decided")
    picks = np.zeros(8, np.uint32)
    a, used = C.c_int32(0), C.c_int32(0)
    check_error(lib().kjarni_lookup_accept_sampled(_f(lg), ld, rows, vocab, d.ctypes.data_as(_ffi._u32p) if d.size else None, d.size,
                                                   temperature, -1 if top_k is None else top_k, -1.0 if top_p is None else top_p,
                                                   -1.0 if min_p is None else min_p, _f(u), picks.ctypes.data_as(_ffi._u32p), C.byref(a),
                                                   C.byref(used)))
    return picks[:a.value + 1].tolist(), int(a.value), int(used.value)


def topk(scores, k: int, device: int = 0):
    """Top-k of a score matrix [nq, n] on the GPU (kjarni_hip_cosine_topk): (idx int64 [nq,k], score f32 [nq,k]),
    score descending, equal scores by ascending index; entries past n are (-1, -inf)."""
    import ctypes as C
    from ._ffi import check_error
    scores = np.ascontiguousarray(scores, np.float32)
    if scores.ndim == 1:
        scores = scores[None, :]
    nq, n = scores.shape
    L = lib()
    ws_bytes = L.kjarni_hip_cosine_topk_workspace_bytes(nq, n, k)
    bufs = []

    def dmalloc(nbytes):
        p = C.c_void_p()
        check_error(L.kjarni_hip_malloc(device, max(nbytes, 16), C.byref(p)))
        bufs.append(p)
        return p
    try:
        d_sc, d_ws, d_idx, d_out = dmalloc(scores.nbytes), dmalloc(ws_bytes), dmalloc(nq * k * 8), dmalloc(nq * k * 4)
        check_error(L.kjarni_hip_memcpy_h2d(device, d_sc, scores.ctypes.data_as(C.c_void_p), scores.nbytes))
        check_error(L.kjarni_hip_cosine_topk(device, d_sc, nq, n, k, d_ws, d_idx, d_out, None))
        check_error(L.kjarni_hip_synchronize(device))
        idx = np.empty((nq, k), np.int64)
        out = np.empty((nq, k), np.float32)
        check_error(L.kjarni_hip_memcpy_d2h(device, idx.ctypes.data_as(C.c_void_p), d_idx, idx.nbytes))
        check_error(L.kjarni_hip_memcpy_d2h(device, out.ctypes.data_as(C.c_void_p), d_out, out.nbytes))
        return idx, out
    finally:
        for p in bufs:
            L.kjarni_hip_free(device, p)



def score_head(hidden, W, targets, bf16=False, slab_tiles=0, fused=True, device=0):
    """The scoring head kernels alone (kjarni_hip_op_score_head): hidden f32 [m, k] (final-normed rows), W [vocab, k] f32, or
    with bf16=True its bf16 bits (uint16); targets [m].  Returns (logprob f32 [m], top u32 [m], top_logprob f32 [m], lse f32 [m]).
    fused: the matrix-core kernel that never stores the logits (slab_tiles 64-wide vocabulary tiles per workgroup, 0 =
    automatic); else the rows route over logits materialised 8 rows at a time."""
    import ctypes as C
    from ._ffi import check_error
    hidden = np.ascontiguousarray(hidden, np.float32)
    W = np.ascontiguousarray(W, np.uint16 if bf16 else np.float32)
    targets = np.ascontiguousarray(targets, np.uint32)
    m, k = hidden.shape
    vocab = W.shape[0]
    if W.shape[1] != k or targets.shape != (m,):
        raise ValueError("hidden [m, k], W [vocab, k], targets [m]")
    lp, top, tlp, lse = np.empty(m, np.float32), np.empty(m, np.uint32), np.empty(m, np.float32), np.empty(m, np.float32)
    f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    check_error(lib().kjarni_hip_op_score_head(device, f(hidden), m, k, W.ctypes.data_as(C.c_void_p), 1 if bf16 else 0, vocab, u32(targets),
                                               slab_tiles, 1 if fused else 0, f(lp), u32(top), f(tlp), f(lse)))
    return lp, top, tlp, lse


def score_head_topk(hidden, W, targets, top_k, bf16=False, slab_tiles=0, fused=True, device=0):
    """score_head with the top_k (1 .. 8, <= vocab) largest logits of every row (kjarni_hip_op_score_head_topk).  Returns
    (logprob f32 [m], topk_ids u32 [m, top_k], topk_logprob f32 [m, top_k], lse f32 [m]); slot j holds the j-th largest logit's
    column and log-probability (equal logits: the larger column first).  logprob, lse and slot 0 are score_head's bits."""
    import ctypes as C
    from ._ffi import check_error
    hidden = np.ascontiguousarray(hidden, np.float32)
    W = np.ascontiguousarray(W, np.uint16 if bf16 else np.float32)
    targets = np.ascontiguousarray(targets, np.uint32)
    m, k = hidden.shape
    vocab = W.shape[0]
    if W.shape[1] != k or targets.shape != (m,):
        raise ValueError("hidden [m, k], W [vocab, k], targets [m]")
    kk = max(int(top_k), 0)
    lp, lse = np.empty(m, np.float32), np.empty(m, np.float32)
    tid, tlp = np.empty((m, kk), np.uint32), np.empty((m, kk), np.float32)
    f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    check_error(lib().kjarni_hip_op_score_head_topk(device, f(hidden), m, k, W.ctypes.data_as(C.c_void_p), 1 if bf16 else 0, vocab,
                                                    u32(targets), slab_tiles, 1 if fused else 0, int(top_k), f(lp), u32(tid), f(tlp), f(lse)))
    return lp, tid, tlp, lse


def wide_rope_scatter(qkv, n_heads: int, n_kv_heads: int, head_dim: int, cos_t, sin_t, k_cache, v_cache, capacity: int, pos, live,
                      rotate: bool = True, gamma_q=None, gamma_k=None, eps: float = 0.0, device: int = 0):
    """One launch_lane_rope_scatter (gamma_q / gamma_k given: launch_lane_qk_norm_rope_scatter, the Qwen3 form) over the 64-lane state on host arrays
    (kjarni_hip_op_wide_rope_scatter).  qkv [lanes, ld] holds Q | K | V of each lane's new token; k_cache / v_cache
    [lanes, lane rows, kv] (lane rows >= capacity).  Returns copies (qkv, k_cache, v_cache) after the call: Q rotated in place,
    K rotated (rotate False: copied) and V copied to row pos[lane] of the lane's caches, nothing for a lane with live == 0 or
    pos >= capacity."""
    q = np.array(qkv, np.float32, order="C")
    kc, vc = np.array(k_cache, np.float32, order="C"), np.array(v_cache, np.float32, order="C")
    if q.ndim != 2 or kc.ndim != 3 or kc.shape != vc.shape or kc.shape[0] != q.shape[0]:
        raise ValueError("qkv [lanes, ld]; k_cache and v_cache [lanes, lane rows, kv]")
    lanes = q.shape[0]
    ps, lv = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(live, np.int32)
    ct, st = _c(cos_t), _c(sin_t)
    if ps.size != lanes or lv.size != lanes or ct.shape != st.shape or ct.ndim != 2:
        raise ValueError("pos / live [lanes]; cos_t / sin_t [table rows, head_dim / 2]")
    gq, gk = _c(gamma_q), _c(gamma_k)
    check_error(lib().kjarni_hip_op_wide_rope_scatter(device, _f(q), q.shape[1], lanes, int(n_heads), int(n_kv_heads), int(head_dim), _f(gq),
                                                      _f(gk), float(eps), _f(ct), _f(st), ct.shape[0], _f(kc), _f(vc),
                                                      kc.shape[1] * kc.shape[2], int(capacity), ps.ctypes.data_as(_i32p),
                                                      lv.ctypes.data_as(_i32p), int(bool(rotate))))
    return q, kc, vc


def wide_pick(logits, state: "_ffi.KjarniHipWideState", history, capacity: int, lanes: Optional[int] = None, first_lane: int = 0,
              advance: bool = True, vocab: Optional[int] = None, device: int = 0):
    """One launch_lane_pick over the 64-lane state (kjarni_hip_op_wide_pick) over lanes [first_lane, first_lane + lanes) of logits [rows, ld]: `state` is
    updated in place; returns the history [64, stride] after the call (a copy)."""
    lg = np.ascontiguousarray(logits, np.float32)
    hist = np.array(history, np.int32, order="C")
    if lg.ndim != 2 or hist.ndim != 2 or hist.shape[0] != 64:
        raise ValueError("logits [rows, ld]; history [64, stride]")
    lanes = lg.shape[0] - first_lane if lanes is None else int(lanes)
    if first_lane < 0 or lanes < 0 or first_lane + lanes > lg.shape[0]:
        raise ValueError("logits must hold rows [0, first_lane + lanes)")
    check_error(lib().kjarni_hip_op_wide_pick(device, _f(lg), lg.shape[1], lg.shape[1] if vocab is None else int(vocab), lanes, int(first_lane),
                                              C.byref(state), hist.ctypes.data_as(_i32p), hist.shape[1], int(capacity), int(bool(advance))))
    return hist
