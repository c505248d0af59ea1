"""Float64 reference of the dense (f32 / bf16) decode-step projections -- launch_llm_gemv, launch_llm_gemv_lanes and
launch_llm_qkv_rope (llm_kernels.hip) -- in plain numpy, each operation stated once, and the three launchers' route rules restated
in Python (llm_gemv_route, llm_gemv_lanes_route, llm_qkv_rope_route), which the GPU tests hold against the route the launcher
itself reports.  No GPU, no library call."""
import math
from typing import Optional

import numpy as np

F64 = np.float64

STREAM, SPLITK, ONE, GENERIC = 0, 1, 2, 3          # llm_gemv_route's kernel
PAIR, QKV_STREAM, QKV_STREAM_EMBED = 0, 1, 2       # llm_qkv_rope_route's kernel
STREAM_K = (2048, 4096, 8192)


# ---- the operations -------------------------------------------------------------------------------------------------------------------

def widen(w: np.ndarray, bf16: bool = False) -> np.ndarray:
    """Weights as float64: f32, or bf16 bit patterns (uint16) widened exactly."""
    if bf16:
        return (np.ascontiguousarray(w, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(F64)
    return np.asarray(w, np.float32).astype(F64)


def rms_norm64(x, gamma, eps: float) -> np.ndarray:
    x = np.asarray(x, F64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + float(eps)) * np.asarray(gamma, F64)


def layer_norm64(x, gamma, beta, eps: float) -> np.ndarray:
    x = np.asarray(x, F64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + float(eps)) * np.asarray(gamma, F64) + np.asarray(beta, F64)


def silu64(g) -> np.ndarray:
    g = np.asarray(g, F64)
    return g / (1.0 + np.exp(-g))


def gelu_tanh64(v) -> np.ndarray:
    v = np.asarray(v, F64)
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def dot64(xn: np.ndarray, w: np.ndarray, bf16: bool = False, block: int = 2048) -> np.ndarray:
    """xn [rows, k] (float64) . w [n, k]^T, the weights widened a block of rows at a time."""
    out = np.empty((xn.shape[0], w.shape[0]), F64)
    for i in range(0, w.shape[0], block):
        out[:, i:i + block] = xn @ widen(w[i:i + block], bf16).T
    return out


def gemv64(x, w, gamma=None, beta=None, eps: float = 0.0, layernorm: bool = False, gelu_tanh: bool = False, w2=None,
           swiglu: bool = False, bias=None, r=None, bf16: bool = False) -> np.ndarray:
    """y [rows, n_out] = epi(norm(x) . w^T + bias): x [rows, k] the rows and columns the call uses, r [rows, n_out]."""
    xn = np.asarray(x, np.float32).astype(F64)
    if layernorm:
        xn = layer_norm64(xn, gamma, beta, eps)
    elif gamma is not None:
        xn = rms_norm64(xn, gamma, eps)
    y = dot64(xn, w, bf16)
    if bias is not None:
        y = y + np.asarray(bias, np.float32).astype(F64)
    if swiglu:
        y = silu64(y) * dot64(xn, w2, bf16)
    if gelu_tanh:
        y = gelu_tanh64(y)
    if r is not None:
        y = y + np.asarray(r, np.float32).astype(F64)
    return y


def segments(y: np.ndarray, seg_q: int, seg_kv: int):
    """The segment scatter: columns [0, seg_q) -> Y0 at row r, the next seg_kv -> Y1 and the last seg_kv -> Y2 at row row_off + r."""
    return y[:, :seg_q], y[:, seg_q:seg_q + seg_kv], y[:, seg_q + seg_kv:seg_q + 2 * seg_kv]


def rope64(v, n_heads: int, head_dim: int, cos_row, sin_row) -> np.ndarray:
    """Pairs (i, i + d/2) of every head rotated by one row of the tables [d/2]."""
    h = np.asarray(v, F64).reshape(n_heads, head_dim)
    half = head_dim // 2
    c, s = np.asarray(cos_row, np.float32).astype(F64), np.asarray(sin_row, np.float32).astype(F64)
    a, b = h[:, :half], h[:, half:]
    return np.concatenate([a * c - b * s, a * s + b * c], axis=1).reshape(-1)


def embed_row(table, idx: int, bf16: bool = False) -> np.ndarray:
    """Row idx of the table as f32 (exact for either dtype); zeros for idx >= vocab."""
    vocab, k = table.shape
    if idx >= vocab:
        return np.zeros(k, np.float32)
    return widen(table[idx], bf16).astype(np.float32)


def qkv_rope64(x, gamma, eps: float, w, bias, n_heads: int, n_kv_heads: int, head_dim: int, cos_t, sin_t, pos: int,
               bf16: bool = False):
    """(Q [n_heads * d], K row, V row [n_kv_heads * d]) of one token at position pos."""
    y = gemv64(np.asarray(x, np.float32)[None, :], w, gamma=gamma, eps=eps, bias=bias, bf16=bf16)[0]
    qd, kvd = n_heads * head_dim, n_kv_heads * head_dim
    q = rope64(y[:qd], n_heads, head_dim, cos_t[pos], sin_t[pos])
    k = rope64(y[qd:qd + kvd], n_kv_heads, head_dim, cos_t[pos], sin_t[pos])
    return q, k, y[qd + kvd:qd + 2 * kvd].copy()


# ---- the route rules, restated ------------------------------------------------------------------------------------------------------

def _stream_rows(ch: int, lpp: int, nm: int, wide: bool) -> int:
    return 16 // (ch * lpp * nm) if wide and 16 // (ch * lpp * nm) > 1 else 1


def gemv_route(rows: int, k: int, n_out: int, bf16: bool = False, norm: bool = False, layernorm: bool = False, gelu_tanh: bool = False,
               swiglu: bool = False, seg_q: int = 0, att_splits: int = 0) -> dict:
    """llm_gemv_route for 16-byte aligned operands: kernel, ch, wide, threads, loop, rows_per_batch, workgroups."""
    r = dict(kernel=GENERIC, ch=0, wide=0, threads=256, loop=0, rows_per_batch=1, workgroups=(n_out + 3) // 4)
    if not layernorm and rows == 1 and seg_q == 0 and k in STREAM_K:
        ch, nm, lpp = k // 512, 2 if swiglu else 1, 1 if bf16 else 2
        wide = n_out // _stream_rows(ch, lpp, nm, True) >= 2048
        rb = _stream_rows(ch, lpp, nm, wide)
        batches = -(-n_out // rb)
        big = batches >= 2048 and (ch >= 16 or att_splits > 0)
        wpw = 8 if big else 4
        loop = -(-batches // wpw) > 4096 // wpw
        form_wide = wide or loop
        return dict(kernel=STREAM, ch=ch, wide=int(form_wide), threads=512 if big else 256, loop=int(loop),
                    rows_per_batch=_stream_rows(ch, lpp, nm, form_wide), workgroups=2048 // wpw if loop else max(1, -(-batches // wpw)))
    ln_splitk = layernorm and rows == 1 and gelu_tanh and seg_q == 0 and k <= 2048
    ln_one = layernorm and rows == 1 and not gelu_tanh and k <= 16384
    rms_splitk = not layernorm and rows == 1 and seg_q == 0 and k <= 16384
    rms_one = not layernorm and rows == 1 and norm and k <= 16384
    if ln_splitk or (not ln_one and rms_splitk):
        wide = not ln_splitk and k >= 8192
        threads = 1024 if wide else 256
        chunks = -(-(k // 8) // threads)
        ch = 1 if chunks <= 1 else 2 if chunks <= 2 else 4 if chunks <= 4 else 8
        return dict(kernel=SPLITK, ch=1 if ln_splitk else min(ch, 2) if wide else ch, wide=int(wide), threads=threads, loop=0,
                    rows_per_batch=2, workgroups=(n_out + 1) // 2)
    if ln_one or rms_one:
        r.update(kernel=ONE, rows_per_batch=2, workgroups=(n_out + 7) // 8)
    return r


def lanes_route(rows: int, k: int, n_out: int, bf16: bool = False, swiglu: bool = False, norm_out: bool = False) -> dict:
    """llm_gemv_lanes_route for 16-byte aligned operands and ldx % 4 == 0: taken, ch, ns, wide, cpw, workgroups."""
    if not (1 <= rows <= 8 and k >= 512 and k % 8 == 0 and not norm_out):
        return dict(taken=0, ch=0, ns=0, wide=0, cpw=0, workgroups=0)
    lpp, nm = 1 if bf16 else 2, 2 if swiglu else 1
    ch = 2 if -(-k // 1024) * 1024 - k < -(-k // 2048) * 2048 - k else 4
    ns = -(-k // (ch * 512))
    cpw_wide = max(1, min(4, 16 // (ch * lpp * nm)))
    wide = -(-n_out // (4 * cpw_wide)) >= 512
    cpw = cpw_wide if wide else 1
    nb = -(-n_out // (4 * cpw))
    return dict(taken=1, ch=ch, ns=ns, wide=int(wide), cpw=cpw, workgroups=min(nb, 512) if ns == 1 else nb)


def qkv_route(k: int, n_heads: int, n_kv_heads: int, head_dim: int, embed: bool = False) -> dict:
    """llm_qkv_rope_route for a 16-byte aligned w and a gamma: kernel, ch, workgroups."""
    tasks = (n_heads + 2 * n_kv_heads) * head_dim // 2
    if k in STREAM_K:
        return dict(kernel=QKV_STREAM_EMBED if embed else QKV_STREAM, ch=k // 512, workgroups=(tasks + 3) // 4)
    chunks = -(-(k // 8) // 256)
    return dict(kernel=PAIR, ch=1 if chunks <= 1 else 2 if chunks <= 2 else 4, workgroups=tasks)


def bar(ref: np.ndarray, rel: Optional[float] = 1e-5) -> float:
    """The project's bar for these kernels: 1e-5 x max(1, max |ref|)."""
    return rel * max(1.0, float(np.abs(ref).max()))
