"""Token-level access to the decoder-only (Llama / Qwen2) path on the GPU (kjarni_hip_decoder_*)."""
from __future__ import annotations

import ctypes as C
import json
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import check_error, lib

WEIGHTS = {"auto": 0, "f32": 1, "bf16": 2}
WEIGHT_TYPE_F8_E4M3 = 31  # KJARNI_HIP_WEIGHT_TYPE_F8_E4M3: the FP8 codes' entry in weight_bytes_by_type


def prefix_keep(resident: Sequence[int], prompt: Sequence[int], limit: int) -> int:
    """The prefix-reuse rule (no GPU): min(longest common prefix of `resident` and `prompt`, limit) -- the cache rows a call
    keeps when it starts from `prompt` on a cache that holds `resident`."""
    r, p = np.ascontiguousarray(resident, np.uint32), np.ascontiguousarray(prompt, np.uint32)
    keep = C.c_size_t(0)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32)) if x.size else None  # noqa: E731
    check_error(lib().kjarni_hip_prefix_keep(u32(r), r.size, u32(p), p.size, int(limit), C.byref(keep)))
    return int(keep.value)


def generation_replay(n_prompt: int, capacity: int, max_new_tokens: int, stream: Sequence[int], max_len: int = 0,
                      stop_ids: Sequence[int] = (), default_stop_ids: Sequence[int] = (), cancel_after: int = -1,
                      feed_last: bool = False):
    """The bookkeeping rule of the generation loops (no GPU) on a given token stream: (emitted, asked, fed) -- tokens emitted,
    tokens taken from `stream` (the draws of a sampled loop), emitted tokens that are fed to another step.  stop_ids empty:
    default_stop_ids; cancel_after k: the callback returns false at the k-th emitted token; feed_last: the last token of
    max_new_tokens counts as fed (generate()'s processor / sampling loops) or not (the lanes)."""
    arr = [np.ascontiguousarray(x, np.uint32) for x in (stop_ids, default_stop_ids, stream)]
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32)) if x.size else None  # noqa: E731
    e, a, f = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    check_error(lib().kjarni_generation_replay(int(n_prompt), int(capacity), int(max_new_tokens), int(max_len), u32(arr[0]), arr[0].size,
                                               u32(arr[1]), arr[1].size, u32(arr[2]), arr[2].size, int(cancel_after), int(bool(feed_last)),
                                               C.byref(e), C.byref(a), C.byref(f)))
    return int(e.value), int(a.value), int(f.value)


EMBED_CHUNK_ROWS = 2048


def embed_plan(lengths: Sequence[int], head_dim: int = 64):
    """The packing rule of HipDecoder.embed (no GPU): sequences of `lengths` tokens go greedily, in order, into chunks of at most
    EMBED_CHUNK_ROWS rows.  Returns (chunk_first_seq, vec_blocks, mfma_blocks): the first sequence of every chunk followed by
    len(lengths); the query blocks of the vector route (32 rows each) and of the matrix-core route (128 rows each; sequences
    of >= 256 rows with head_dim 64 / 128) as int32 [n, 4] rows (chunk, the sequence's first row in the chunk, the block's first
    query row in the sequence, the sequence's length)."""
    a = np.ascontiguousarray(lengths, np.int32)
    i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    cap = int(np.maximum(a, 0).astype(np.int64).sum() // 32 + a.size + 1)
    first = np.zeros(a.size + 1, np.int32)
    vec, mfma = np.zeros((cap, 4), np.int32), np.zeros((cap, 4), np.int32)
    nc, nv, nm = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check_error(lib().kjarni_hip_embed_plan(i32(a) if a.size else None, a.size, int(head_dim), i32(first), C.byref(nc), i32(vec), cap,
                                            C.byref(nv), i32(mfma), cap, C.byref(nm)))
    return first[:nc.value + 1].copy(), vec[:nv.value].copy(), mfma[:nm.value].copy()


def _flatten(seqs):
    """(ids u32, offsets i32 [n + 1]) of a list of token sequences."""
    n = len(seqs)
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.uint32).reshape(-1) for s in seqs]) if n else [], np.uint32)
    if flat.size == 0:
        flat = np.zeros(1, np.uint32)
    return flat, np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(s) for s in seqs])]), np.int32)


SCORE_MIN_SHARED = 2  # KJARNI_HIP_SCORE_MIN_SHARED: the shortest prefix HipDecoder.score_batch computes once


def score_plan(seqs: Sequence[Sequence[int]], firsts: Sequence[int], head_dim: int = 64, min_shared: int = SCORE_MIN_SHARED) -> dict:
    """The plan of HipDecoder.score_batch (no GPU).  Walking the sequences in order, a sequence gathers the neighbours behind it
    while their common prefix -- capped by every member's `first`, so that it never holds a scored token -- stays at least
    min_shared tokens, the group fits one chunk of EMBED_CHUNK_ROWS rows and every remainder stays below 256 rows; a group
    computes its prefix once.  Returns a dict of int32 arrays: chunk_first_seq [chunks + 1], chunk_rows [chunks], groups [n, 4]
    (chunk, first sequence, members, prefix length), vec / mfma [n, 4] (chunk, first row, first query row, length: plain
    sequences and prefixes, embed_plan's rule), prefix [n, 6] (chunk, the remainder's first row, the block's first query row,
    the remainder's length, the prefix's first row, the prefix length: 32 query rows each) and gather [n, 4] (chunk, the chunk
    row of position pos - 1, the target id, the output slot: one per scored position)."""
    flat, off = _flatten(seqs)
    fs = np.ascontiguousarray(firsts, np.int32)
    n = len(seqs)
    if fs.size != n:
        raise ValueError("one `first` per sequence")
    i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    total = int(max(off[-1], 0))
    cap = total + n + 1
    first, rows = np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.int32)
    groups, vec, mfma = np.zeros((n + 1, 4), np.int32), np.zeros((cap, 4), np.int32), np.zeros((cap, 4), np.int32)
    pre, gather = np.zeros((cap, 6), np.int32), np.zeros((cap, 4), np.int32)
    cnt = [C.c_int32(0) for _ in range(6)]
    check_error(lib().kjarni_hip_score_plan(flat.ctypes.data_as(C.POINTER(C.c_uint32)) if n else None, i32(off) if n else None,
                                            i32(fs) if n else None, n, int(head_dim), int(min_shared), i32(first), i32(rows), C.byref(cnt[0]),
                                            i32(groups), n + 1, C.byref(cnt[1]), i32(vec), cap, C.byref(cnt[2]), i32(mfma), cap,
                                            C.byref(cnt[3]), i32(pre), cap, C.byref(cnt[4]), i32(gather), cap, C.byref(cnt[5])))
    nc, ng, nv, nm, np_, nga = (c.value for c in cnt)
    return {"chunk_first_seq": first[:nc + 1].copy(), "chunk_rows": rows[:nc].copy(), "groups": groups[:ng].copy(), "vec": vec[:nv].copy(),
            "mfma": mfma[:nm].copy(), "prefix": pre[:np_].copy(), "gather": gather[:nga].copy()}


ANSWER_MAX_TARGETS = 8  # KJARNI_HIP_ANSWER_MAX_TARGETS


def answer_plan(seqs: Sequence[Sequence[int]], head_dim: int = 64, min_shared: int = SCORE_MIN_SHARED) -> dict:
    """The plan of HipDecoder.answer_logits (no GPU): score_plan's rule and tables with every sequence's `first` at its last token,
    so that no shared prefix holds a sequence's last token.  The dict is score_plan's, but gather is [n, 3]: per sequence, in
    order, (chunk, the chunk row of its last token, the sequence's index)."""
    flat, off = _flatten(seqs)
    n = len(seqs)
    i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    cap = int(max(off[-1], 0)) + n + 1
    first, rows = np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.int32)
    groups, vec, mfma = np.zeros((n + 1, 4), np.int32), np.zeros((cap, 4), np.int32), np.zeros((cap, 4), np.int32)
    pre, gather = np.zeros((cap, 6), np.int32), np.zeros((n + 1, 3), np.int32)
    cnt = [C.c_int32(0) for _ in range(6)]
    check_error(lib().kjarni_hip_answer_plan(flat.ctypes.data_as(C.POINTER(C.c_uint32)) if n else None, i32(off) if n else None, n, int(head_dim),
                                             int(min_shared), i32(first), i32(rows), C.byref(cnt[0]), i32(groups), n + 1, C.byref(cnt[1]),
                                             i32(vec), cap, C.byref(cnt[2]), i32(mfma), cap, C.byref(cnt[3]), i32(pre), cap, C.byref(cnt[4]),
                                             i32(gather), n + 1, C.byref(cnt[5])))
    nc, ng, nv, nm, np_, nga = (c.value for c in cnt)
    return {"chunk_first_seq": first[:nc + 1].copy(), "chunk_rows": rows[:nc].copy(), "groups": groups[:ng].copy(), "vec": vec[:nv].copy(),
            "mfma": mfma[:nm].copy(), "prefix": pre[:np_].copy(), "gather": gather[:nga].copy()}


LOGPROB_GUARD = 8  # entries the generate_*_logprobs wrappers allocate behind the capacity they pass on (a test hook)


class HipDecoder:
    def __init__(self, model_dir: str, device: int = 0, weights: str = "auto", max_context: int = 0):
        self._h = C.c_void_p()
        self._lanes = 0  # set by lanes_begin()
        check_error(lib().kjarni_hip_decoder_load(model_dir.encode("utf-8"), device, WEIGHTS[weights], max_context, C.byref(self._h)))
        a, b, c, d, e = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        wb = C.c_uint64()
        check_error(lib().kjarni_hip_decoder_dims(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(wb)))
        self.hidden, self.layers, self.vocab, self.context, self.bf16, self.weight_bytes = a.value, b.value, c.value, d.value, bool(e.value), wb.value
        cfg = json.loads(self.config_json())  # config.json, or the config synthesized from a GGUF file's metadata
        self.config = cfg
        heads = cfg["num_attention_heads"] if "num_attention_heads" in cfg else cfg["n_head"]  # (GPT-2's field name)
        self.kv_heads = cfg.get("num_key_value_heads", heads)
        self.head_dim = cfg.get("head_dim", self.hidden // heads)

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().kjarni_hip_decoder_free(self._h)
            self._h = C.c_void_p()

    def config_json(self) -> str:
        """The resolved model config as JSON."""
        p = C.c_void_p()
        check_error(lib().kjarni_hip_decoder_config_json(self._h, C.byref(p)))
        s = C.string_at(p).decode("utf-8")
        lib().kjarni_string_free(p)
        return s

    def weight_bytes_by_type(self) -> dict:
        """Device bytes of the weights per type name (F32, BF16, Q8_0, Q4_K, Q6_K; F8_E4M3: the codes of an FP8 checkpoint, whose
        scales count as F32), non-zero entries only."""
        out = (C.c_uint64 * 32)()
        check_error(lib().kjarni_hip_decoder_weight_bytes_by_type(self._h, out, 32))
        names = {0: "F32", 8: "Q8_0", 12: "Q4_K", 14: "Q6_K", 30: "BF16", WEIGHT_TYPE_F8_E4M3: "F8_E4M3"}
        return {names[t]: int(out[t]) for t in names if out[t]}

    def reset(self):
        check_error(lib().kjarni_hip_decoder_reset(self._h))

    def set_device_sampling(self, on: bool):
        lib().kjarni_hip_decoder_set_device_sampling(self._h, 1 if on else 0)

    def tile_gemm_calls(self) -> int:
        """Prompt projections that took the 128 x 128-tile GEMM route since load."""
        return int(lib().kjarni_hip_decoder_tile_gemm_calls(self._h))

    def cache_len(self) -> int:
        """Positions held in the KV cache."""
        return int(lib().kjarni_hip_decoder_cache_len(self._h))

    def kv_rows(self, layer: int, first: int = 0, rows: Optional[int] = None):
        """Cache rows [first, first + rows) of `layer` (default: to the end of the cache): (K after RoPE, V), each f32
        [rows, kv_heads * head_dim]."""
        if rows is None:
            rows = self.cache_len() - first
        if rows < 0:
            raise ValueError("first is past the end of the cache")
        kv = self.kv_heads * self.head_dim
        k, v = np.empty((rows, kv), np.float32), np.empty((rows, kv), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_kv_rows(self._h, layer, first, rows, f(k), f(v)))
        return k, v

    def moe_routing(self, layer: int):
        """What sparse layer `layer` of a qwen3_moe decoder chose in its last pass: (ids int32 [rows, k], weights f32 [rows, k]),
        slot 0 the largest weight.  A dense layer or a dense model raises (InvalidConfig)."""
        n = C.c_int32(0)
        check_error(lib().kjarni_hip_decoder_moe_routing(self._h, layer, 0, C.byref(n), None, None))
        k = int(json.loads(self.config_json()).get("num_experts_per_tok", 1))
        ids, w = np.empty((n.value, k), np.int32), np.empty((n.value, k), np.float32)
        check_error(lib().kjarni_hip_decoder_moe_routing(self._h, layer, n.value, C.byref(n), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         w.ctypes.data_as(C.POINTER(C.c_float))))
        return ids[:n.value], w[:n.value]

    def forward(self, ids: Sequence[int], fetch: bool = True):
        a = np.ascontiguousarray(ids, np.uint32)
        hidden = np.empty(((a.size - 1) % 8 + 1, self.hidden), np.float32) if fetch else None   # rows of the last 8-row block
        logits = np.empty(self.vocab, np.float32) if fetch else None
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float)) if x is not None else None  # noqa: E731
        check_error(lib().kjarni_hip_decoder_forward(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size, f(hidden), f(logits)))
        return hidden, logits

    def generate(self, prompt: Sequence[int], max_new_tokens: int, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                 on_token: Optional[Callable[[int], Optional[bool]]] = None) -> List[int]:
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate(self._h, p.ctypes.data_as(C.POINTER(C.c_uint32)), p.size, max_new_tokens,
                                                      repetition_penalty, no_repeat_ngram, fn, None,
                                                      out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)))
        return out[:min(n.value, out.size)].tolist()

    # ---- lanes: up to 8 prompts decoded in lock step ----
    def generate_batch(self, prompts: Sequence[Sequence[int]], max_new_tokens, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                       lanes: int = 0, lane_context: int = 0,
                       on_token: Optional[Callable[[int, int], Optional[bool]]] = None) -> List[List[int]]:
        """generate() for every prompt, up to `lanes` (1..8, 0 = 8) of them at a time, each in a KV cache of `lane_context` rows
        (<= 0: the decoder's context).  max_new_tokens: one int for all prompts, or one per prompt.  on_token(prompt index, token)
        is called in step order, lane order within a step; returning False ends that prompt only."""
        return self._generate_many(lib().kjarni_hip_decoder_generate_batch, prompts, max_new_tokens, repetition_penalty, no_repeat_ngram, lanes,
                                   lane_context, on_token)

    def _generate_many(self, entry, prompts, max_new_tokens, repetition_penalty, no_repeat_ngram, lanes, lane_context, on_token):
        n = len(prompts)
        if n == 0:
            check_error(entry(self._h, None, None, 0, None, repetition_penalty, no_repeat_ngram, lanes,
                              lane_context, _ffi.KjarniBatchTokenCallbackFn(), None, None, 0, None))
            return []
        new = [int(max_new_tokens)] * n if np.isscalar(max_new_tokens) else [int(m) for m in max_new_tokens]
        if len(new) != n:
            raise ValueError("max_new_tokens: one value, or one per prompt")
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32).reshape(-1) for p in prompts]), np.uint32)
        if flat.size == 0:
            flat = np.zeros(1, np.uint32)
        offsets = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in prompts])]).tolist())
        news = (C.c_size_t * n)(*new)
        cap = max(max(new), 1)
        out = np.zeros((n, cap), np.uint32)
        n_out = (C.c_size_t * n)()

        def cb(i, t, _u):
            r = on_token(int(i), int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniBatchTokenCallbackFn(cb) if on_token else _ffi.KjarniBatchTokenCallbackFn()
        check_error(entry(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), offsets, n, news,
                          repetition_penalty, no_repeat_ngram, lanes, lane_context, fn, None,
                          out.ctypes.data_as(C.POINTER(C.c_uint32)), cap, n_out))
        return [out[i, :min(int(n_out[i]), cap)].tolist() for i in range(n)]

    # ---- wide lanes: up to 64 prompts decoded in lock step, the projections on the matrix cores ----
    def generate_wide(self, prompts: Sequence[Sequence[int]], max_new_tokens, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                      lanes: int = 0, lane_context: int = 0,
                      on_token: Optional[Callable[[int, int], Optional[bool]]] = None) -> List[List[int]]:
        """generate_batch() with up to `lanes` (1..64, 0 = 64) prompts at a time.  An effective width min(lanes, len(prompts)) of 8
        or less runs generate_batch's own step; 9..64 runs the wide step (f32 / bf16 safetensors checkpoints).  The lane caches
        take 2 * layers * lanes * rows * kv * 4 bytes with rows = min(context, lane_context): set lane_context."""
        return self._generate_many(lib().kjarni_hip_decoder_generate_wide, prompts, max_new_tokens, repetition_penalty, no_repeat_ngram, lanes,
                                   lane_context, on_token)

    def generate_wide_logprobs(self, prompts: Sequence[Sequence[int]], max_new_tokens, top_k: int = 0, repetition_penalty: float = 1.0,
                               no_repeat_ngram: int = 0, lanes: int = 0, lane_context: int = 0,
                               on_token: Optional[Callable[[int, int], Optional[bool]]] = None, capacity: Optional[int] = None):
        """generate_wide() with the log-probability of every emitted token and its top_k (0..8) alternatives: a list, one dict
        per prompt, of ids, logprob [n], topk_ids / topk_logprob [n, top_k].  Every width 1..64 is served.  The distribution is
        score()'s (the raw logits); a lane that takes the next waiting prompt starts at that prompt's record 0.
        guard (a test hook): as generate_logprobs', per prompt; the last prompt's also holds the LOGPROB_GUARD entries behind the arrays."""
        n = len(prompts)
        if n == 0:
            return []
        new = [int(max_new_tokens)] * n if np.isscalar(max_new_tokens) else [int(m) for m in max_new_tokens]
        if len(new) != n:
            raise ValueError("max_new_tokens: one value, or one per prompt")
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32).reshape(-1) for p in prompts]), np.uint32)
        if flat.size == 0:
            flat = np.zeros(1, np.uint32)
        offsets = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in prompts])]).tolist())
        news = (C.c_size_t * n)(*new)
        cap = max(max(new), 1) if capacity is None else int(capacity)
        k = max(int(top_k), 0)
        # [n, cap] rows as the C entry lays them out, then LOGPROB_GUARD entries the call must not touch (a test hook)
        room = n * cap + LOGPROB_GUARD
        out_f, lp_f = np.full(room, 0xFFFFFFFF, np.uint32), np.full(room, np.nan, np.float32)
        ids_f, tlp_f = np.full((room, k), 0xFFFFFFFF, np.uint32), np.full((room, k), np.nan, np.float32)
        out, lp = out_f[:n * cap].reshape(n, cap), lp_f[:n * cap].reshape(n, cap)
        ids, tlp = ids_f[:n * cap].reshape(n, cap, k), tlp_f[:n * cap].reshape(n, cap, k)
        n_out = (C.c_size_t * n)()

        def cb(i, t, _u):
            r = on_token(int(i), int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniBatchTokenCallbackFn(cb) if on_token else _ffi.KjarniBatchTokenCallbackFn()
        f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_generate_wide_logprobs(self._h, u32(flat), offsets, n, news, repetition_penalty, no_repeat_ngram,
                                                                    lanes, lane_context, fn, None, u32(out_f), cap, n_out, int(top_k), f32(lp_f),
                                                                    u32(ids_f) if k else None, f32(tlp_f) if k else None))
        res = []
        for i in range(n):
            m = min(int(n_out[i]), cap)
            # guard: the entries of the prompt's own rows behind its records; the last prompt's also holds the entries behind the arrays
            tail = slice(n * cap, None) if i == n - 1 else slice(0, 0)
            guard = tuple(np.concatenate([a[i, m:], f[tail]]) for a, f in ((out, out_f), (lp, lp_f), (ids, ids_f), (tlp, tlp_f)))
            res.append({"ids": out[i, :m].tolist(), "n": int(n_out[i]), "logprob": lp[i, :m].copy(), "topk_ids": ids[i, :m].copy(),
                        "topk_logprob": tlp[i, :m].copy(), "guard": guard})
        return res

    def generate_wide_constrained(self, prompts: Sequence[Sequence[int]], max_new_tokens, automata=None, top_k: int = -1,
                                  repetition_penalty: float = 1.0, no_repeat_ngram: int = 0, lanes: int = 0, lane_context: int = 0,
                                  on_token: Optional[Callable[[int, int], Optional[bool]]] = None):
        """generate_wide() with an automaton per prompt: automata[i] is None (the plain behaviour), a constraints.Constraint (a
        pattern) or a constraints.GrammarConstraint; the model's stop ids end a prompt where its automaton accepts.  Returns a list,
        one dict per prompt: ids, result (constraints.lane_result_dict: kind, final_state, device_state, final_depth,
        device_depth, accepted, complete, violated) and, with top_k >= 0, logprob [n], topk_ids / topk_logprob [n, top_k] under
        the raw distribution.  Prompt i's ids and result are those of generate_constrained / generate_grammar / generate on it alone."""
        from .constraints import GrammarConstraint, lane_result_dict
        n = len(prompts)
        if n == 0:
            return []
        automata = [None] * n if automata is None else list(automata)
        if len(automata) != n:
            raise ValueError("automata: one entry per prompt (None: unconstrained)")
        new = [int(max_new_tokens)] * n if np.isscalar(max_new_tokens) else [int(m) for m in max_new_tokens]
        if len(new) != n:
            raise ValueError("max_new_tokens: one value, or one per prompt")
        flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32).reshape(-1) for p in prompts]), np.uint32)
        if flat.size == 0:
            flat = np.zeros(1, np.uint32)
        offsets = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in prompts])]).tolist())
        news = (C.c_size_t * n)(*new)
        cap = max(max(new), 1)
        k = max(int(top_k), 0)
        out, lp = np.full((n, cap), 0xFFFFFFFF, np.uint32), np.full((n, cap), np.nan, np.float32)
        ids, tlp = np.full((n, cap, k), 0xFFFFFFFF, np.uint32), np.full((n, cap, k), np.nan, np.float32)
        n_out = (C.c_size_t * n)()
        cons, grams = (C.c_void_p * n)(), (C.c_void_p * n)()
        for i, a in enumerate(automata):
            if a is None:
                continue
            if isinstance(a, GrammarConstraint):
                grams[i] = a._h.value
            else:
                cons[i] = a._h.value
        results = (_ffi.KjarniHipLaneAutomatonResult * n)()

        def cb(i, t, _u):
            r = on_token(int(i), int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniBatchTokenCallbackFn(cb) if on_token else _ffi.KjarniBatchTokenCallbackFn()
        f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_generate_wide_constrained(self._h, u32(flat), offsets, n, news, repetition_penalty, no_repeat_ngram,
                                                                       lanes, lane_context, fn, None, u32(out), cap, n_out, int(top_k),
                                                                       f32(lp) if top_k >= 0 else None, u32(ids) if k else None,
                                                                       f32(tlp) if k else None, cons, grams, results))
        res = []
        for i in range(n):
            m = min(int(n_out[i]), cap)
            d = {"ids": out[i, :m].tolist(), "result": lane_result_dict(results[i])}
            if top_k >= 0:
                d.update(logprob=lp[i, :m].copy(), topk_ids=ids[i, :m].copy(), topk_logprob=tlp[i, :m].copy())
            res.append(d)
        return res

    def wide_begin(self, lanes: int = 0, lane_context: int = 0):
        """Test hook: empty wide-lane caches for `lanes` (9..64, 0 = 64) lanes of `lane_context` rows each."""
        check_error(lib().kjarni_hip_decoder_wide_begin(self._h, lanes, lane_context))
        self._wide_lanes = lanes or 64

    def wide_prefill(self, lane: int, ids: Sequence[int]):
        a = np.ascontiguousarray(ids, np.uint32)
        check_error(lib().kjarni_hip_decoder_wide_prefill(self._h, lane, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def wide_prefill_shared(self, lane: int, shared: int, ids: Sequence[int]):
        a = np.ascontiguousarray(ids, np.uint32)
        check_error(lib().kjarni_hip_decoder_wide_prefill_shared(self._h, lane, int(shared), a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def wide_step(self, ids: Sequence[int], live: Optional[Sequence[int]] = None):
        """One wide step: lane l appends ids[l] where live[l] (default: every lane).  Returns the final-normed hidden rows
        [lanes, hidden] and the logits [lanes, vocab]; the rows of frozen lanes are unspecified."""
        a = np.ascontiguousarray(ids, np.uint32)
        if a.size != getattr(self, "_wide_lanes", 0):
            raise ValueError("one id per lane (after wide_begin)")
        lv = np.ascontiguousarray(live, np.int32) if live is not None else None
        if lv is not None and lv.size != a.size:
            raise ValueError("one live flag per lane")
        hidden = np.empty((a.size, self.hidden), np.float32)
        logits = np.empty((a.size, self.vocab), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_wide_step(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                       lv.ctypes.data_as(C.POINTER(C.c_int32)) if lv is not None else None, f(hidden), f(logits)))
        return hidden, logits

    def wide_cache_len(self, lane: int) -> int:
        return int(lib().kjarni_hip_decoder_wide_cache_len(self._h, lane))

    def wide_capacity(self) -> int:
        return int(lib().kjarni_hip_decoder_wide_capacity(self._h))

    def wide_kv_rows(self, lane: int, layer: int, first: int = 0, rows: Optional[int] = None):
        """kv_rows() of one wide lane's cache."""
        if rows is None:
            rows = self.wide_cache_len(lane) - first
        if rows < 0:
            raise ValueError("first is past the end of the lane's cache")
        kv = self.kv_heads * self.head_dim
        k, v = np.empty((rows, kv), np.float32), np.empty((rows, kv), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_wide_kv_rows(self._h, lane, layer, first, rows, f(k), f(v)))
        return k, v

    def lanes_begin(self, lanes: int = 0, lane_context: int = 0):
        """Test hook: empty lane caches for `lanes` lanes of `lane_context` rows each."""
        check_error(lib().kjarni_hip_decoder_lanes_begin(self._h, lanes, lane_context))
        self._lanes = lanes or 8

    def lane_prefill(self, lane: int, ids: Sequence[int]):
        a = np.ascontiguousarray(ids, np.uint32)
        check_error(lib().kjarni_hip_decoder_lane_prefill(self._h, lane, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def lanes_step(self, ids: Sequence[int], live: Optional[Sequence[int]] = None):
        """One lock-step step: lane l appends ids[l] where live[l] (default: every lane).  Returns the final-normed hidden rows
        [lanes, hidden] and the logits [lanes, vocab]; the rows of frozen lanes are unspecified."""
        a = np.ascontiguousarray(ids, np.uint32)
        if self._lanes and a.size != self._lanes:
            raise ValueError("one id per lane")
        lv = np.ascontiguousarray(live, np.int32) if live is not None else None
        hidden = np.empty((a.size, self.hidden), np.float32)
        logits = np.empty((a.size, self.vocab), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_lanes_step(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        lv.ctypes.data_as(C.POINTER(C.c_int32)) if lv is not None else None, f(hidden), f(logits)))
        return hidden, logits

    def lane_cache_len(self, lane: int) -> int:
        return int(lib().kjarni_hip_decoder_lane_cache_len(self._h, lane))

    def lane_capacity(self) -> int:
        return int(lib().kjarni_hip_decoder_lane_capacity(self._h))

    def lane_kv_rows(self, lane: int, layer: int, first: int = 0, rows: Optional[int] = None):
        """kv_rows() of one lane's cache."""
        if rows is None:
            rows = self.lane_cache_len(lane) - first
        if rows < 0:
            raise ValueError("first is past the end of the lane's cache")
        kv = self.kv_heads * self.head_dim
        k, v = np.empty((rows, kv), np.float32), np.empty((rows, kv), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_lane_kv_rows(self._h, lane, layer, first, rows, f(k), f(v)))
        return k, v

    def lane_gemv_calls(self):
        """(streamed, fallback): projections of lane steps that took the multi-row weight-streaming kernel / the one-wave-per-
        column kernel since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_lane_gemv_calls(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- prompt-lookup decoding: greedy generation that verifies a draft from its own history every step ----
    def generate_lookup(self, prompt: Sequence[int], max_new_tokens: int, draft_tokens: int = 7, ngram_max: int = 3, ngram_min: int = 1,
                        stop_ids: Optional[Sequence[int]] = None, on_token: Optional[Callable[[int], Optional[bool]]] = None):
        """generate() for a greedy request through the lookup loop: (ids, stats), stats = verify_steps, drafted_tokens,
        accepted_tokens and single_row_steps over the steps the host consumed.  stop_ids (default: config.json's eos ids)
        end the call and are not emitted."""
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)
        cfg = _ffi.KjarniHipLookupConfig(draft_tokens, ngram_max, ngram_min)
        st = _ffi.KjarniHipLookupStats()
        stops = np.ascontiguousarray(stop_ids if stop_ids is not None else [], np.uint32)
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_lookup(self._h, u32(p), p.size, max_new_tokens, u32(stops) if stops.size else None,
                                                             stops.size, C.byref(cfg), fn, None, u32(out), out.size, C.byref(n), C.byref(st)))
        stats = {k: int(getattr(st, k)) for k, _ in _ffi.KjarniHipLookupStats._fields_}
        return out[:min(n.value, out.size)].tolist(), stats

    def verify_step(self, token: int, draft: Sequence[int], rows: Optional[int] = None):
        """Test hook: one verify step of `rows` rows (default len(draft) + 1) on the cache as it stands.  Returns (picks,
        accepted, logits [len(draft) + 1, vocab]); the cache grows by accepted + 1."""
        d = np.ascontiguousarray(draft, np.uint32)
        rows = d.size + 1 if rows is None else int(rows)
        picks = np.zeros(8, np.uint32)
        a = C.c_int32(0)
        logits = np.empty((d.size + 1, self.vocab), np.float32)
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_verify_step(self._h, int(token), u32(d) if d.size else None, d.size, rows, u32(picks), C.byref(a),
                                                         logits.ctypes.data_as(C.POINTER(C.c_float))))
        return picks[:a.value + 1].tolist(), int(a.value), logits

    # ---- prompt-lookup decoding for sampled requests ----
    @staticmethod
    def _sampling_options(max_new_tokens, sample, temperature, top_k, top_p, min_p, repetition_penalty, no_repeat_ngram, stop_ids,
                          uniforms, seed):
        """(KjarniHipSamplingOptions, the arrays it points into)."""
        stops = np.ascontiguousarray(stop_ids if stop_ids is not None else [], np.uint32)
        u = None if uniforms is None else np.ascontiguousarray(uniforms, np.float32)
        o = _ffi.KjarniHipSamplingOptions()
        o.max_new_tokens, o.repetition_penalty, o.no_repeat_ngram, o.sample = max_new_tokens, repetition_penalty, no_repeat_ngram, int(sample)
        o.temperature = temperature
        o.top_k = -1 if top_k is None else top_k
        o.top_p = -1.0 if top_p is None else top_p
        o.min_p = -1.0 if min_p is None else min_p
        o.stop_ids = stops.ctypes.data_as(C.POINTER(C.c_uint32)) if stops.size else None
        o.n_stop = stops.size
        o.uniforms = u.ctypes.data_as(C.POINTER(C.c_float)) if u is not None else None
        o.n_uniforms = 0 if u is None else u.size
        o.seed = seed
        return o, (stops, u)

    def generate_sampled(self, prompt: Sequence[int], max_new_tokens: int, lookup: Optional[Sequence[int]] = None, sample: bool = True,
                         temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                         min_p: Optional[float] = None, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                         stop_ids: Optional[Sequence[int]] = None, uniforms=None, seed: int = 0,
                         on_token: Optional[Callable[[int], Optional[bool]]] = None):
        """generate() with a sampling strategy: (ids, stats).  lookup None: the plain loop; (draft_tokens, ngram_max, ngram_min):
        the sampled lookup loop, which returns the plain loop's ids for the same draws.  uniforms: token i uses uniforms[i]
        (at least max_new_tokens of them); None: a generator seeded with `seed`."""
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)
        o, keep = self._sampling_options(max_new_tokens, sample, temperature, top_k, top_p, min_p, repetition_penalty, no_repeat_ngram,
                                         stop_ids, uniforms, seed)
        cfg = None if lookup is None else _ffi.KjarniHipLookupConfig(*[int(x) for x in lookup])
        st = _ffi.KjarniHipLookupStats()
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_sampled(self._h, u32(p) if p.size else None, p.size, C.byref(o),
                                                              C.byref(cfg) if cfg is not None else None, fn, None, u32(out), out.size,
                                                              C.byref(n), C.byref(st)))
        del keep
        stats = {k: int(getattr(st, k)) for k, _ in _ffi.KjarniHipLookupStats._fields_}
        return out[:min(n.value, out.size)].tolist(), stats

    def generate_constrained(self, constraint, prompt: Sequence[int], max_new_tokens: int, sample: bool = False,
                             temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                             min_p: Optional[float] = None, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                             stop_ids: Optional[Sequence[int]] = None, uniforms=None, seed: int = 0,
                             on_token: Optional[Callable[[int], Optional[bool]]] = None):
        """generate() / generate_sampled()'s plain loop under a kjarni_amd.constraints.Constraint: (ids, result).  After every
        token the bytes of the emitted tokens are a prefix of a string the pattern matches in full; in an accepting state the
        stop ids are legal; a closed state ends the run without a stop token.  result: final_state, device_state, accepted,
        complete, violated (kjarni_hip.h: KjarniHipConstraintResult)."""
        from .constraints import result_dict
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)
        o, keep = self._sampling_options(max_new_tokens, sample, temperature, top_k, top_p, min_p, repetition_penalty, no_repeat_ngram,
                                         stop_ids, uniforms, seed)
        res = _ffi.KjarniHipConstraintResult()
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_constrained(self._h, constraint._h if constraint is not None else None,
                                                                  u32(p) if p.size else None, p.size, C.byref(o), fn, None, u32(out), out.size,
                                                                  C.byref(n), C.byref(res)))
        del keep
        return out[:min(n.value, out.size)].tolist(), result_dict(res)

    def generate_grammar(self, grammar, prompt: Sequence[int], max_new_tokens: int, sample: bool = False, temperature: float = 1.0,
                         top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                         repetition_penalty: float = 1.0, no_repeat_ngram: int = 0, stop_ids: Optional[Sequence[int]] = None,
                         uniforms=None, seed: int = 0, on_token: Optional[Callable[[int], Optional[bool]]] = None):
        """generate_constrained() under a kjarni_amd.constraints.GrammarConstraint (a stack automaton in the DFA's place):
        (ids, result).  After every token the bytes of the emitted tokens are a prefix of a string of the grammar; in an accepted
        configuration the stop ids are legal; a closed configuration ends the run without a stop token.  result: final_state,
        final_depth, device_state, device_depth, accepted, complete, violated (kjarni_hip.h: KjarniHipGrammarResult)."""
        from .constraints import grammar_result_dict
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)
        o, keep = self._sampling_options(max_new_tokens, sample, temperature, top_k, top_p, min_p, repetition_penalty, no_repeat_ngram,
                                         stop_ids, uniforms, seed)
        res = _ffi.KjarniHipGrammarResult()
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_grammar(self._h, grammar._h if grammar is not None else None,
                                                              u32(p) if p.size else None, p.size, C.byref(o), fn, None, u32(out), out.size,
                                                              C.byref(n), C.byref(res)))
        del keep
        return out[:min(n.value, out.size)].tolist(), grammar_result_dict(res)

    def generate_logprobs(self, prompt: Sequence[int], max_new_tokens: int, top_k: int = 0, constraint=None, grammar=None,
                          sample: bool = False, temperature: float = 1.0, sampling_top_k: Optional[int] = None,
                          top_p: Optional[float] = None, min_p: Optional[float] = None, repetition_penalty: float = 1.0,
                          no_repeat_ngram: int = 0, stop_ids: Optional[Sequence[int]] = None, uniforms=None, seed: int = 0,
                          on_token: Optional[Callable[[int], Optional[bool]]] = None, capacity: Optional[int] = None):
        """The plain loop of generate_sampled() / generate_constrained() / generate_grammar() with the log-probability of every
        emitted token and its top_k (0..8) most likely alternatives: a dict with ids, logprob [n], topk_ids / topk_logprob
        [n, top_k] and result (the constraint's or grammar's, else None).  The distribution is score()'s: the log-softmax of the
        logits as the vocabulary head wrote them, before the mask, the processors, temperature and the sampler's cut.
        sampling_top_k is the sampler's cut (generate_sampled's top_k).  capacity: the size of the output arrays (default
        max_new_tokens); the records cover the first min(n, capacity) tokens.  n: the tokens emitted; guard (a test hook): every
        output array is allocated LOGPROB_GUARD entries longer than the capacity the C entry is told, filled with 0xFFFFFFFF /
        NaN; guard holds the entries of each array behind min(n, capacity), which the call must leave as they were."""
        from .constraints import grammar_result_dict, result_dict
        p = np.ascontiguousarray(prompt, np.uint32)
        cap = max(max_new_tokens, 1) if capacity is None else int(capacity)
        k = max(int(top_k), 0)
        room = max(cap, 0) + LOGPROB_GUARD
        out = np.full(room, 0xFFFFFFFF, np.uint32)
        lp = np.full(room, np.nan, np.float32)
        ids = np.full((room, k), 0xFFFFFFFF, np.uint32)
        tlp = np.full((room, k), np.nan, np.float32)
        n = C.c_size_t(0)
        o, keep = self._sampling_options(max_new_tokens, sample, temperature, sampling_top_k, top_p, min_p, repetition_penalty,
                                         no_repeat_ngram, stop_ids, uniforms, seed)
        cres, gres = _ffi.KjarniHipConstraintResult(), _ffi.KjarniHipGrammarResult()
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_logprobs(
            self._h, constraint._h if constraint is not None else None, grammar._h if grammar is not None else None,
            u32(p) if p.size else None, p.size, C.byref(o), int(top_k), fn, None, u32(out), cap, C.byref(n), f32(lp),
            u32(ids) if ids.size else None, f32(tlp) if tlp.size else None, C.byref(cres), C.byref(gres)))
        del keep
        m = min(n.value, cap)
        result = result_dict(cres) if constraint is not None else grammar_result_dict(gres) if grammar is not None else None
        return {"ids": out[:m].tolist(), "n": int(n.value), "logprob": lp[:m].copy(), "topk_ids": ids[:m].copy(),
                "topk_logprob": tlp[:m].copy(), "result": result, "guard": (out[m:], lp[m:], ids[m:], tlp[m:])}

    def verify_step_sampled(self, token: int, draft: Sequence[int], uniforms, rows: Optional[int] = None, temperature: float = 1.0,
                            top_k: Optional[int] = None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                            repetition_penalty: float = 1.0, history: Optional[Sequence[int]] = None, fetch: bool = True):
        """Test hook: verify_step() for a sampled request, one draw per decided row.  history: the tokens the penalty counts, ending
        with `token` (needed when repetition_penalty != 1).  Returns (picks, accepted, draws_used, processed logits
        [len(draft) + 1, vocab], or None with fetch=False); the cache grows by accepted + 1."""
        d = np.ascontiguousarray(draft, np.uint32)
        u = np.ascontiguousarray(uniforms, np.float32)
        h = np.ascontiguousarray(history if history is not None else [], np.uint32)
        if u.size < d.size + 1:
            raise ValueError("one draw per row that may be decided")
        rows = d.size + 1 if rows is None else int(rows)
        o, keep = self._sampling_options(0, True, temperature, top_k, top_p, min_p, repetition_penalty, 0, None, None, 0)
        picks = np.zeros(8, np.uint32)
        a, used = C.c_int32(0), C.c_int32(0)
        logits = np.empty((d.size + 1, self.vocab), np.float32) if fetch else None
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_verify_step_sampled(self._h, int(token), u32(d) if d.size else None, d.size, rows, C.byref(o),
                                                                 u32(h) if h.size else None, h.size,
                                                                 u.ctypes.data_as(C.POINTER(C.c_float)), u32(picks), C.byref(a),
                                                                 C.byref(used), logits.ctypes.data_as(C.POINTER(C.c_float)) if fetch else None))
        del keep
        return picks[:a.value + 1].tolist(), int(a.value), int(used.value), logits

    def sampling_routes(self):
        """(tokens decided from the device's candidates, tokens that needed a logits row) since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_sampling_routes(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def verify_gemv_calls(self):
        """(streamed, fallback): projections of verify steps that took the multi-row weight-streaming kernel / the
        one-wave-per-column kernel since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_verify_gemv_calls(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- speculative decoding with a draft model ----
    def generate_draft(self, draft: "HipDecoder", prompt: Sequence[int], max_new_tokens: int, draft_tokens: int, sample: bool = False,
                       temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None,
                       min_p: Optional[float] = None, repetition_penalty: float = 1.0, no_repeat_ngram: int = 0,
                       stop_ids: Optional[Sequence[int]] = None, uniforms=None, seed: int = 0,
                       on_token: Optional[Callable[[int], Optional[bool]]] = None):
        """generate() / generate_sampled() with `draft`, a second HipDecoder on the same device with the same vocabulary,
        proposing draft_tokens (1..7, required) tokens per verify step: (ids, stats).  Every emitted token is this decoder's
        own decision, so the ids are the plain loop's for the same options and draws; the drafter only changes the speed.
        Greedy with a penalty, or any n-gram ban, takes the plain loop (stats zero)."""
        p = np.ascontiguousarray(prompt, np.uint32)
        out = np.empty(max(max_new_tokens, 1), np.uint32)
        n = C.c_size_t(0)
        o, keep = self._sampling_options(max_new_tokens, sample, temperature, top_k, top_p, min_p, repetition_penalty, no_repeat_ngram,
                                         stop_ids, uniforms, seed)
        st = _ffi.KjarniHipLookupStats()
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731

        def cb(t, _u):
            r = on_token(int(t.token_id))
            return True if r is None else bool(r)
        fn = _ffi.KjarniTokenCallbackFn(cb) if on_token else _ffi.KjarniTokenCallbackFn()
        check_error(lib().kjarni_hip_decoder_generate_draft(self._h, draft._h if draft is not None else None, u32(p) if p.size else None,
                                                            p.size, C.byref(o), int(draft_tokens), fn, None, u32(out), out.size,
                                                            C.byref(n), C.byref(st)))
        del keep
        stats = {k: int(getattr(st, k)) for k, _ in _ffi.KjarniHipLookupStats._fields_}
        return out[:min(n.value, out.size)].tolist(), stats

    def draft_round(self, draft: "HipDecoder", token: int, rows: int, fetch: bool = True):
        """Test hook: one greedy round of `rows` (2..8) rows on the two caches as they stand; `token` is in neither.  Returns
        (proposals [rows - 1], picks, accepted, logits [rows, vocab] or None with fetch=False); this cache grows by
        accepted + 1, the drafter's ends there or one row short (every proposal accepted)."""
        rows = int(rows)
        proposals = np.zeros(7, np.uint32)
        picks = np.zeros(8, np.uint32)
        a = C.c_int32(0)
        logits = np.empty((max(rows, 1), self.vocab), np.float32) if fetch else None
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_draft_round(self._h, draft._h if draft is not None else None, int(token), rows, u32(proposals),
                                                         u32(picks), C.byref(a),
                                                         logits.ctypes.data_as(C.POINTER(C.c_float)) if fetch else None))
        return proposals[:max(rows - 1, 0)].tolist(), picks[:a.value + 1].tolist(), int(a.value), logits

    # ---- scoring: per-token log-probabilities of a given sequence ----
    def score(self, ids: Sequence[int], first: int = 1):
        """Resets the cache, runs `ids` and returns, for the positions first .. len(ids) - 1: (log p(ids[p] | ids[:p]) f32, the
        arg-max token of that distribution u32, the arg-max's log-probability f32), len(ids) - first entries each.  Leaves the
        decoder as reset() + forward(ids) does."""
        a = np.ascontiguousarray(ids, np.uint32)
        cnt = max(a.size - int(first), 0)
        lp, top, tlp = np.empty(cnt, np.float32), np.empty(cnt, np.uint32), np.empty(cnt, np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_score(self._h, u32(a), a.size, int(first), f(lp), u32(top), f(tlp)))
        return lp, top, tlp

    def score_topk(self, ids: Sequence[int], first: int = 1, top_k: int = 8):
        """score() with the top_k (1 .. 8, not above the vocabulary) most likely tokens of every scored position: (logprob f32
        [cnt], ids u32 [cnt, top_k], logprob f32 [cnt, top_k]) with cnt = len(ids) - first.  Slot j of a row is the token with
        the j-th largest logit (equal logits: the larger id first); slot 0 is score()'s arg-max, and the first array is
        score()'s, bit for bit.  Same routes, counters and final state as score()."""
        a = np.ascontiguousarray(ids, np.uint32)
        cnt, k = max(a.size - int(first), 0), max(int(top_k), 0)
        lp, tid, tlp = np.empty(cnt, np.float32), np.empty((cnt, k), np.uint32), np.empty((cnt, k), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_score_topk(self._h, u32(a), a.size, int(first), int(top_k), f(lp), u32(tid), f(tlp)))
        return lp, tid, tlp

    def set_score_fused(self, on: bool):
        """On (the default): f32 / bf16 heads are scored on the matrix cores without storing the logits; off: every checkpoint
        takes the rows route (8 materialised logits rows at a time)."""
        lib().kjarni_hip_decoder_set_score_fused(self._h, 1 if on else 0)

    def score_calls(self):
        """(fused, rows): head launches of score() by route since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_score_calls(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- scoring many sequences in one packed pass ----
    def score_batch(self, seqs: Sequence[Sequence[int]], firsts: Sequence[int], top_k: int = 1):
        """score() / score_topk() for every sequence in one packed pass: the scored positions of sequence b are firsts[b] ..
        len(seqs[b]) - 1.  Returns (logprob f32 [S], ids u32 [S, top_k], logprob f32 [S, top_k]) with S = sum(len - first), flat in
        sequence order then position order (np.split at np.cumsum(len - first) gives them per sequence); slot 0 of a row is
        score()'s arg-max.  Neighbouring sequences that start with the same tokens compute them once (score_plan); the KV cache and
        everything generate() and score() depend on are left as they were."""
        flat, off = _flatten(seqs)
        return self.score_batch_flat(flat, off, firsts, top_k)

    def score_batch_flat(self, ids, offsets, firsts, top_k: int = 1):
        """score_batch() on ids, offsets [n + 1] and firsts [n] as the C ABI takes them."""
        a, o = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(offsets, np.int32)
        fs = np.ascontiguousarray(firsts, np.int32)
        n = o.size - 1
        if fs.size != n:
            raise ValueError("one `first` per sequence")
        cnt = int(np.maximum(np.diff(o.astype(np.int64)) - fs, 0).sum()) if n > 0 else 0
        k = max(int(top_k), 0)
        lp, tid, tlp = np.zeros(cnt, np.float32), np.zeros((cnt, k), np.uint32), np.zeros((cnt, k), np.float32)
        f = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        i32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        check_error(lib().kjarni_hip_decoder_score_batch(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), i32(o), n, i32(fs) if n > 0 else None,
                                                         int(top_k), f(lp), tid.ctypes.data_as(C.POINTER(C.c_uint32)), f(tlp)))
        return lp, tid, tlp

    def score_batch_rows(self):
        """(computed, saved): rows score_batch() ran through the layer stack, and prefix rows it did not compute a second time,
        since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_score_batch_rows(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- answer logits: a few chosen logits at the end of many sequences ----
    def answer_logits(self, seqs: Sequence[Sequence[int]], targets: Sequence[int]) -> np.ndarray:
        """f32 [len(seqs), len(targets)]: the logit of every target token (1 .. ANSWER_MAX_TARGETS ids, shared by the batch) at the
        position after each sequence's last token, in one packed pass without the vocabulary head.  Neighbouring sequences that
        start with the same tokens compute them once, their last tokens excepted (answer_plan); the KV cache and everything
        generate(), score() and score_batch() depend on are left as they were."""
        flat, off = _flatten(seqs)
        return self.answer_logits_flat(flat, off, targets)

    def answer_logits_flat(self, ids, offsets, targets) -> np.ndarray:
        """answer_logits() on ids and offsets [n + 1] as the C ABI takes them."""
        a, o = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(offsets, np.int32)
        t = np.ascontiguousarray(targets, np.uint32).reshape(-1)
        n = o.size - 1
        buf = np.zeros(max(n * t.size, 1), np.float32)
        u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        tp = u32(t) if t.size else u32(np.zeros(1, np.uint32))
        check_error(lib().kjarni_hip_decoder_answer_logits(self._h, u32(a), o.ctypes.data_as(C.POINTER(C.c_int32)), n, tp, t.size,
                                                           buf.ctypes.data_as(C.POINTER(C.c_float))))
        return buf[:max(n, 0) * t.size].reshape(max(n, 0), t.size)

    def answer_rows(self):
        """(computed, saved): rows answer_logits() ran through the layer stack, and prefix rows it did not compute a second time,
        since load (score_batch_rows() counts its own calls only)."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_answer_rows(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- embedding: last-token pooling over a packed batch ----
    def embed(self, sequences: Sequence[Sequence[int]], normalize: bool = True) -> np.ndarray:
        """[len(sequences), hidden]: the final-normed hidden state of every sequence's last token, L2-normalised when
        `normalize`.  All sequences run packed through the prompt routes in chunks of at most EMBED_CHUNK_ROWS rows; the KV cache
        and everything generate() depends on are left as they were."""
        n = len(sequences)
        out = np.zeros((n, self.hidden), np.float32)
        lens = [len(s) for s in sequences]
        flat = np.ascontiguousarray(np.concatenate([np.asarray(s, np.uint32).reshape(-1) for s in sequences]) if n else [], np.uint32)
        if flat.size == 0:
            flat = np.zeros(1, np.uint32)
        offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)]), np.int32)
        self.embed_flat(flat, offsets, normalize, out)
        return out

    def embed_flat(self, ids, offsets, normalize: bool = True, out: Optional[np.ndarray] = None) -> np.ndarray:
        """embed() on ids and offsets [n + 1] as the C ABI takes them (sequence b = ids[offsets[b]:offsets[b + 1]])."""
        a, o = np.ascontiguousarray(ids, np.uint32), np.ascontiguousarray(offsets, np.int32)
        n = o.size - 1
        if out is None:
            out = np.zeros((n, self.hidden), np.float32)
        check_error(lib().kjarni_hip_decoder_embed(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), o.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                   int(bool(normalize)), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    # ---- prefix reuse: keep the cached rows of the tokens a call shares with what the cache holds ----
    def set_prefix_reuse(self, on: bool):
        """Off (the default): generate*, score and generate_batch prefill whole prompts.  On: they keep the cache rows of
        prefix_keep(resident(), prompt, limit) -- limit len(prompt) - 1, score: first - 1 -- and forward the rest;
        generate_batch prefills the prefix its prompts share once and copies its rows into the lanes."""
        lib().kjarni_hip_decoder_set_prefix_reuse(self._h, 1 if on else 0)

    # ---- FP8 checkpoints on the matrix cores ----
    def set_fp8_matrix_cores(self, on: bool):
        """Off (the default): an FP8 checkpoint's prompt projections dequantize each matrix to f32 first, and more than 8 lanes
        refuse it.  On: the prompt GEMM multiplies the FP8 codes themselves on the bf16 matrix cores (launch_prefill_gemm_fp8) and
        generate_wide / the wide hooks accept the checkpoint.  A no-op on a checkpoint that is not FP8."""
        lib().kjarni_hip_decoder_set_fp8_matrix_cores(self._h, 1 if on else 0)

    def fp8_matrix_cores(self) -> bool:
        return bool(lib().kjarni_hip_decoder_fp8_matrix_cores(self._h))

    def prefix_stats(self):
        """(reused, computed): prompt tokens whose rows were kept / computed by the calls that ran with reuse on, since load."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_decoder_prefix_stats(self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def resident(self) -> List[int]:
        """Test hook: the tokens behind cache rows [0, len(result)); never longer than cache_len()."""
        n = C.c_size_t(0)
        check_error(lib().kjarni_hip_decoder_resident(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        check_error(lib().kjarni_hip_decoder_resident(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(n)))
        return out[:n.value].tolist()

    def last_logits(self):
        """Test hook: the logits row the last forward of the single-sequence path left on the device."""
        out = np.empty(self.vocab, np.float32)
        check_error(lib().kjarni_hip_decoder_last_logits(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def lane_prefill_shared(self, lane: int, shared: int, ids: Sequence[int]):
        """Test hook (after lanes_begin): rows [0, shared) of the single-sequence cache copied into `lane`, then `ids` prefilled
        behind them."""
        a = np.ascontiguousarray(ids, np.uint32)
        check_error(lib().kjarni_hip_decoder_lane_prefill_shared(self._h, lane, int(shared), a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))
