"""Plain numpy references for the encoder's packed-row kernels (rowops.hip, attention.hip on `cu`): float64 where a bar is held,
float32 restatements in the kernel's own operation order where bit-exactness is claimed, and launch_attention's route rule
restated from the text of attention.hip (not by calling it)."""
import numpy as np

F32, F64 = np.float32, np.float64

# attention.hip's kernels, as kjarni_hip.h numbers them
NOTHING, SPLIT, PIPE_PADDED, PIPE_PACKED, PIPE_SHORT, CHUNKED, GENERIC = range(7)
POOL_MEAN, POOL_CLS, POOL_MAX, POOL_LAST = range(4)


def cu_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


# ---- the route ---------------------------------------------------------------------------------------------------------------------

def attention_route(batch, seq, heads, head_dim, aligned=True, packed=False):
    """(kernel, grid).  launch_attention: nothing for an empty call; the any-shape kernel unless head_dim is 32 or 64 and the
    operands are aligned; launch_d: the chunked kernel above 128 keys, the small-call kernel up to 128 (sentence, head) items, else
    an item per workgroup on min(items, 256 * (3 at head_dim 32, 2 at 64)) workgroups -- MODE 1 on packed rows, MODE 2 on padded
    rows of up to 96 tokens, MODE 0 otherwise.  grid is 0 for every kernel but the last three."""
    if batch <= 0 or seq <= 0:
        return NOTHING, 0
    if head_dim not in (32, 64) or not aligned:
        return GENERIC, 0
    if seq > 128:
        return CHUNKED, 0
    items = batch * heads
    if items <= 128:
        return SPLIT, 0
    grid = min(items, 256 * (2 if head_dim == 64 else 3))
    return (PIPE_PACKED if packed else (PIPE_SHORT if seq <= 96 else PIPE_PADDED)), grid


# ---- lengths and the pack index ----------------------------------------------------------------------------------------------------

def mask_lengths(mask):
    """lens[b] = kept tokens; bit 31 when mask[b, 0] == 0 or a value is > 1."""
    mask = np.asarray(mask, np.uint32)
    out = np.zeros(mask.shape[0], np.uint32)
    for b in range(mask.shape[0]):
        count, bad = 0, int(mask[b, 0]) == 0
        for s in range(mask.shape[1]):
            v = int(mask[b, s])
            count += v != 0
            bad = bad or v > 1
        out[b] = count | (0x80000000 if bad else 0)
    return out


def pack_index(mask):
    """(cu [B + 1], tok_src [cu[B]]): the kept tokens of every sentence in ascending position, sentence after sentence."""
    mask = np.asarray(mask, np.uint32)
    B, S = mask.shape
    cu, src = [0], []
    for b in range(B):
        for s in range(S):
            if int(mask[b, s]) != 0:
                src.append(b * S + s)
        cu.append(len(src))
    return np.array(cu, np.int32), np.array(src, np.int32)


# ---- embedding ---------------------------------------------------------------------------------------------------------------------

def embed_f32(ids, word, pos, type_emb, type_ids, seq, vocab, max_pos, type_vocab, pos_offset, scale, src):
    """The embedding sum in the kernel's order, in float32: word[id] (zeros when id >= vocab), * sqrt(H) when scaling,
    + pos[offset + s] when offset + s < max_pos, + type[ty] (row 0 without type ids).  src: the padded index of every output row."""
    ids = np.asarray(ids, np.uint32).reshape(-1)
    H = word.shape[1]
    out = np.zeros((len(src), H), F32)
    sc = np.sqrt(F32(H)).astype(F32)
    for t, i in enumerate(np.asarray(src, np.int64)):
        s = int(i) % seq
        x = np.zeros(H, F32)
        if int(ids[i]) < vocab:
            x = word[int(ids[i])].astype(F32).copy()
        if scale:
            x = (x * sc).astype(F32)
        if pos is not None and pos_offset + s < max_pos:
            x = (x + pos[pos_offset + s]).astype(F32)
        if type_emb is not None and type_vocab > 0:
            ty = 0 if type_ids is None else int(np.asarray(type_ids, np.uint32).reshape(-1)[i])
            x = (x + type_emb[ty]).astype(F32)
        out[t] = x
    return out


def layer_norm(x, gamma, beta, eps):
    """(x - mean) / sqrt(var + eps) * gamma + beta, population variance, float64."""
    x = np.asarray(x, F64)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + F64(eps)) * np.asarray(gamma, F64) + np.asarray(beta, F64)


# ---- RoPE --------------------------------------------------------------------------------------------------------------------------

def rope_f32(qkv, cos, sin, heads, head_dim, positions):
    """Q and K thirds rotated in float32 with two roundings per product-difference (the kernel's __fmul_rn / __fsub_rn); V untouched.
    positions [rows]: the table row of every qkv row."""
    out = np.array(qkv, F32)
    rows = out.shape[0]
    half, hidden = head_dim // 2, heads * head_dim
    p = np.asarray(positions, np.int64)
    c = np.asarray(cos, F32)[p][:, :half]          # [rows, half]
    s = np.asarray(sin, F32)[p][:, :half]
    for part in range(2):
        v = out[:, part * hidden:(part + 1) * hidden].reshape(rows, heads, head_dim)
        x0, x1 = v[:, :, :half].copy(), v[:, :, half:].copy()
        cc, ss = c[:, None, :], s[:, None, :]
        y0 = ((x0 * cc).astype(F32) - (x1 * ss).astype(F32)).astype(F32)
        y1 = ((x0 * ss).astype(F32) + (x1 * cc).astype(F32)).astype(F32)
        v[:, :, :half], v[:, :, half:] = y0, y1
        out[:, part * hidden:(part + 1) * hidden] = v.reshape(rows, hidden)
    return out


# ---- attention ---------------------------------------------------------------------------------------------------------------------

def attention_packed(qkv, lengths, heads, head_dim):
    """softmax(Q K^T / sqrt(d)) V per sentence over its cu rows, no mask, float64.  Returns ctx [cu[B], hidden]."""
    cu = cu_of(lengths)
    H = heads * head_dim
    x = np.asarray(qkv, F64)
    out = np.zeros((int(cu[-1]), H), F64)
    for b in range(len(cu) - 1):
        r0, r1 = int(cu[b]), int(cu[b + 1])
        n = r1 - r0
        q = x[r0:r1, :H].reshape(n, heads, head_dim).transpose(1, 0, 2)
        k = x[r0:r1, H:2 * H].reshape(n, heads, head_dim).transpose(1, 0, 2)
        v = x[r0:r1, 2 * H:3 * H].reshape(n, heads, head_dim).transpose(1, 0, 2)
        s = q @ k.transpose(0, 2, 1) / np.sqrt(F64(head_dim))
        s -= s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(axis=-1, keepdims=True)
        out[r0:r1] = (p @ v).transpose(1, 0, 2).reshape(n, H)
    return out


# ---- pooling -----------------------------------------------------------------------------------------------------------------------

def pool_packed(hs, lengths, mode, normalize):
    """Four modes over the cu rows (every row a kept token), float64; optionally L2-normalised.  A division happens only when the
    count / the norm is > 0."""
    cu = cu_of(lengths)
    x = np.asarray(hs, F64)
    out = np.zeros((len(cu) - 1, x.shape[1]), F64)
    for b in range(len(cu) - 1):
        rows = x[int(cu[b]):int(cu[b + 1])]
        if mode == POOL_MEAN:
            v = rows.sum(axis=0)
            if len(rows) > 0:
                v = v / len(rows)
        elif mode == POOL_CLS:
            v = rows[0]
        elif mode == POOL_MAX:
            v = np.maximum(rows.max(axis=0), -1e9)
        else:
            v = rows[-1]
        if normalize:
            n = np.sqrt((v * v).sum())
            if n > 0:
                v = v / n
        out[b] = v
    return out


def pool_padded(hs, mask, mode, normalize):
    """The padded form under a 0 / 1 mask [B, S]: mean over kept rows (token 0 when none is kept), CLS, max over kept rows with
    -1e9 for the others, the last kept row (0 when none)."""
    x, m = np.asarray(hs, F64), np.asarray(mask, np.int64)
    B, S, H = x.shape
    out = np.zeros((B, H), F64)
    for b in range(B):
        kept = np.nonzero(m[b])[0]
        if mode == POOL_MEAN:
            v = x[b, kept].sum(axis=0) / len(kept) if len(kept) else x[b, 0]
        elif mode == POOL_CLS:
            v = x[b, 0]
        elif mode == POOL_MAX:
            v = np.maximum(x[b, kept].max(axis=0), -1e9) if len(kept) else np.full(H, -1e9)
        else:
            v = x[b, kept[-1] if len(kept) else 0]
        if normalize:
            n = np.sqrt((v * v).sum())
            if n > 0:
                v = v / n
        out[b] = v
    return out


# ---- heads -------------------------------------------------------------------------------------------------------------------------

def small_linear(feat, w, bias, k):
    y = np.asarray(feat, F64)[:, :k] @ np.asarray(w, F64).T
    return y if bias is None else y + np.asarray(bias, F64)


def row_softmax(x, sigmoid):
    x = np.asarray(x, F64)
    if sigmoid:
        return 1.0 / (1.0 + np.exp(-x))
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)
