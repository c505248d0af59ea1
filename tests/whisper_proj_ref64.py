"""Float64 reference of the Whisper decoder's row projections (launch_gemv_rows) and of the front-end kernels (mel_frames,
mel_power, mel_log_normalize, im2col3, add_rows, decoder_embed: whisper_kernels.hip) in plain numpy, each operation stated once,
and launch_gemv_rows' route rule restated in Python, which the tests hold against the route the launcher itself reports.
No GPU, no library call."""
import math

import numpy as np

F32, F64 = np.float32, np.float64

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL = 0, 1, 5
NOTHING, ONE_FAST, ONE_FAST_EMBED, STAGED_FAST, HEAD, STAGED, GENERAL, GEMM, REFUSED = range(9)
MIS_X, MIS_W, MIS_GAMMA, MIS_BETA = 1, 2, 4, 8
PAIRS = ((EPI_BIAS, True), (EPI_BIAS, False), (EPI_BIAS_GELU, True), (EPI_BIAS_RESIDUAL, False))   # (epilogue, LayerNorm)

_erf = np.vectorize(math.erf, otypes=[F64])


def bar(ref) -> float:
    return 1e-5 * max(1.0, float(np.abs(np.asarray(ref, F64)).max()))


# ---- the projections ------------------------------------------------------------------------------------------------------------------

def layer_norm64(x, gamma, beta, eps: float) -> np.ndarray:
    """Two passes: the mean, then the mean of the squared distances from it; eps inside the square root."""
    x = np.asarray(x, F64)
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + float(eps)) * np.asarray(gamma, F32).astype(F64) + np.asarray(beta, F32).astype(F64)


def gelu_erf64(v) -> np.ndarray:
    v = np.asarray(v, F64)
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gemv_rows64(x, w, gamma=None, beta=None, eps: float = 0.0, bias=None, epi: int = EPI_BIAS, r=None) -> np.ndarray:
    """y [rows, n_out] = epi(LN?(x) . w^T + bias) (+ r): x [rows, k] the rows and columns the call uses, r [rows, n_out]."""
    xn = np.asarray(x, F32).astype(F64)
    if gamma is not None:
        xn = layer_norm64(xn, gamma, beta, eps)
    y = xn @ np.asarray(w, F32).astype(F64).T
    if bias is not None:
        y = y + np.asarray(bias, F32).astype(F64)
    if epi == EPI_BIAS_GELU:
        y = gelu_erf64(y)
    if epi == EPI_BIAS_RESIDUAL:
        y = y + np.asarray(r, F32).astype(F64)
    return y


def segments(y: np.ndarray, seg: int):
    """The segment split: columns [0, seg) -> Y0 at row r, [seg, 2 seg) -> Y1 and [2 seg, 3 seg) -> Y2 at row row_off + r."""
    return y[:, :seg], y[:, seg:2 * seg], y[:, 2 * seg:3 * seg]


def embed64(word, idx: int, scale: float, pos_table, p: int) -> np.ndarray:
    """word[idx] * scale + pos_table[p] in float64; zeros for idx >= vocab, nothing added for p >= max_pos or without a table."""
    word = np.asarray(word, F32)
    v = np.zeros(word.shape[1], F64)
    if 0 <= idx < word.shape[0]:
        v = word[idx].astype(F64) * float(F32(scale))
    if pos_table is not None and 0 <= p < len(pos_table):
        v = v + np.asarray(pos_table, F32)[p].astype(F64)
    return v


def embed32(word, idx: int, scale: float, pos_table, p: int) -> np.ndarray:
    """The same with one f32 multiply and one f32 addition, each correctly rounded: what a kernel that does nothing else must give
    bit for bit."""
    word = np.asarray(word, F32)
    v = np.zeros(word.shape[1], F32)
    if 0 <= idx < word.shape[0]:
        v = word[idx] * F32(scale)
    if pos_table is not None and 0 <= p < len(pos_table):
        v = v + np.asarray(pos_table, F32)[p]
    return v.astype(F32)


def decoder_embed32(ids, word, pos_table, offset: int, scale_embeddings: bool, lanes: bool) -> np.ndarray:
    """out[s] = word[ids[s]] * (sqrt(hidden) when scaled) + pos[offset + s] (lanes: offset for every row)."""
    word = np.asarray(word, F32)
    scale = np.sqrt(F32(word.shape[1])) if scale_embeddings else F32(1.0)
    return np.stack([embed32(word, int(i), scale, pos_table, offset + (0 if lanes else s)) for s, i in enumerate(ids)])


# ---- the route rule, restated ---------------------------------------------------------------------------------------------------------

def route(rows: int, n_out: int, k: int, ldx=None, seg: int = 0, epi: int = EPI_BIAS, gamma: bool = False, beta=None, r=None,
          embed: bool = False, x_raw_out: bool = False, x_norm_out: bool = False, misalign: int = 0) -> int:
    """gemv_rows_route for arguments given as sizes and flags (beta defaults to gamma, r to what the epilogue needs; misalign: the
    operands that start 4 bytes past a 16-byte boundary)."""
    ldx = k if ldx is None else ldx
    beta = gamma if beta is None else beta
    r = (epi == EPI_BIAS_RESIDUAL) if r is None else r
    if rows <= 0 or n_out <= 0:
        return NOTHING
    ln = bool(gamma)
    if (ln and not beta) or (epi == EPI_BIAS_RESIDUAL and not r):
        return REFUSED
    if seg > 0 and n_out > 3 * seg:
        return REFUSED
    if (x_raw_out and not embed) or (x_norm_out and not ln):   # no kernel would write them
        return REFUSED
    x_ok, w_ok = not (misalign & MIS_X), not (misalign & MIS_W)
    norm_ok = not ((gamma and misalign & MIS_GAMMA) or (beta and misalign & MIS_BETA))
    wide = k in (512, 2048)
    if embed or x_raw_out or x_norm_out:           # the extras: the one-row kernel alone
        if not (rows == 1 and wide and (not ln or norm_ok) and w_ok and (embed or (ldx % 4 == 0 and x_ok))):
            return REFUSED
    if (epi, ln) not in PAIRS:
        return REFUSED
    if rows > 8 or k % 4 or ldx % 4 or not x_ok or not w_ok:
        return GEMM if not ln and seg <= 0 else REFUSED
    fast = wide and norm_ok
    if rows == 1 and fast:
        if embed:
            return ONE_FAST_EMBED if ln and epi == EPI_BIAS and k == 512 else REFUSED
        return ONE_FAST
    staged = rows >= 2 and rows * k * 4 <= 64 * 1024
    if staged and fast:
        return HEAD if (not ln and epi == EPI_BIAS and seg <= 0 and n_out >= 8192 and k == 512) else STAGED_FAST
    return STAGED if staged else GENERAL


# ---- the front end --------------------------------------------------------------------------------------------------------------------

def pad_reflect(audio, pad: int) -> np.ndarray:
    """numpy's 'reflect' padding with the reference's clamps for signals shorter than the pad: on the left audio[pad], ...,
    audio[1] (an index at or past the end becomes the last sample), on the right audio[n - 2], audio[n - 3], ... (an index before
    the start becomes the first)."""
    a = np.asarray(audio, F32)
    n = len(a)
    left = [a[i if i < n else n - 1] for i in range(pad, 0, -1)]
    right = [a[n - 2 - i if n >= 2 + i else 0] for i in range(pad)]
    return np.concatenate([np.asarray(left, F32), a, np.asarray(right, F32)])


def mel_frames64(audio, window, hop: int, n_frames: int, ld: int) -> np.ndarray:
    """frames [n_frames, ld]: frame f holds padded[f * hop + i] * window[i] for i < n_fft; a frame that would run past the padded
    signal, and every column from n_fft on, is zero."""
    w = np.asarray(window, F32).astype(F64)
    n_fft = len(w)
    padded = pad_reflect(audio, n_fft // 2).astype(F64)
    out = np.zeros((n_frames, ld), F64)
    for f in range(n_frames):
        if f * hop + n_fft > len(padded):
            break
        out[f, :n_fft] = padded[f * hop:f * hop + n_fft] * w
    return out


def mel_power64(dft, im_off: int, n_bins: int, ld_out: int) -> np.ndarray:
    d = np.asarray(dft, F32).astype(F64)
    out = np.zeros((d.shape[0], ld_out), F64)
    out[:, :n_bins] = np.sqrt(d[:, :n_bins] ** 2 + d[:, im_off:im_off + n_bins] ** 2) ** 2
    return out


def mel_power32(dft, im_off: int, n_bins: int, ld_out: int) -> np.ndarray:
    """The same in f32, every operation rounded once: sqrt(re * re + im * im), then the square."""
    d = np.asarray(dft, F32)
    re, im = d[:, :n_bins], d[:, im_off:im_off + n_bins]
    mag = np.sqrt((re * re).astype(F32) + (im * im).astype(F32), dtype=F32)
    out = np.zeros((d.shape[0], ld_out), F32)
    out[:, :n_bins] = mag * mag
    return out


def mel_log64(mel, n_mels: int) -> np.ndarray:
    """log10(max(x, 1e-10)) over the first n_mels columns (the floor is the f32 nearest to 1e-10)."""
    return np.log10(np.maximum(np.asarray(mel, F32)[:, :n_mels].astype(F64), float(F32(1e-10))))


def mel_log_normalize64(mel, n_mels: int):
    """(log, out): out = (max(log, max(log) - 8) + 4) / 4."""
    lg = mel_log64(mel, n_mels)
    return lg, (np.maximum(lg, lg.max() - 8.0) + 4.0) / 4.0


def im2col3_64(x, channels: int, stride: int, pad: int, t_out: int, ld_cols: int) -> np.ndarray:
    """cols [t_out, ld_cols]: column j * channels + c of row t is x[t * stride + j - pad, c], zero outside the rows of x; columns
    from 3 * channels on are zero."""
    x = np.asarray(x, F32)
    out = np.zeros((t_out, ld_cols), F32)
    for t in range(t_out):
        for j in range(3):
            ti = t * stride + j - pad
            if 0 <= ti < x.shape[0]:
                out[t, j * channels:(j + 1) * channels] = x[ti, :channels]
    return out


def add_rows32(x, period: int, table, table_rows: int) -> np.ndarray:
    """x[r] + table[r % period] where r % period < table_rows (one f32 addition), x[r] elsewhere."""
    out = np.array(x, F32)
    t = np.asarray(table, F32)
    for r in range(out.shape[0]):
        if r % period < table_rows:
            out[r] = out[r] + t[r % period]
    return out
