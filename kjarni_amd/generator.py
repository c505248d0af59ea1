"""Raw text completion over the kjarni_generator_* C ABI (the reference's Rust Generator,
crates/kjarni/src/generator/*): no chat template, the output as generated."""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import KjarniDevice, check_error, lib
from .chat import GenerationConfig, ResolvedGeneration, _gen, _resolved, _stream_cb, _take_string


class Generator:
    def __init__(self, model: str, model_path: Optional[str] = None, cache_dir: Optional[str] = None, device: str = "cpu",
                 quiet: bool = True):
        cfg = lib().kjarni_generator_config_default()
        cfg.device = KjarniDevice.GPU if device == "gpu" else KjarniDevice.CPU
        self._keep = [s.encode("utf-8") if s is not None else None for s in (cache_dir, model, model_path)]
        cfg.cache_dir, cfg.model_name, cfg.model_path = self._keep
        cfg.quiet = int(quiet)
        self._handle = C.c_void_p()
        check_error(lib().kjarni_generator_new(C.byref(cfg), C.byref(self._handle)))

    def close(self):
        if getattr(self, "_handle", None) and self._handle.value:
            lib().kjarni_generator_free(self._handle)
            self._handle = C.c_void_p()

    __del__ = close

    @property
    def model_name(self) -> str:
        need = lib().kjarni_generator_model_name(self._handle, None, 0)
        buf = C.create_string_buffer(need + 1)
        lib().kjarni_generator_model_name(self._handle, buf, need + 1)
        return buf.value.decode("utf-8")

    @property
    def context_size(self) -> int:
        return int(lib().kjarni_generator_context_size(self._handle))

    @property
    def vocab_size(self) -> int:
        return int(lib().kjarni_generator_vocab_size(self._handle))

    def generate(self, prompt: str, config: Optional[GenerationConfig] = None) -> str:
        out = C.c_void_p()
        check_error(lib().kjarni_generator_generate(self._handle, prompt.encode("utf-8"), _gen(config), C.byref(out)))
        return _take_string(out)

    def score(self, context: str, continuation: str):
        """(sum_logprob, n_tokens, is_greedy) of `continuation` after `context`: the tokens encode(context + continuation)
        adds to encode(context); an empty context is the BOS token alone."""
        r = _ffi.KjarniScoreResult()
        check_error(lib().kjarni_generator_score(self._handle, context.encode("utf-8"), continuation.encode("utf-8"), C.byref(r)))
        return float(r.sum_logprob), int(r.n_tokens), bool(r.is_greedy)

    def score_batch(self, pairs: Sequence[Sequence[str]]):
        """score() for every (context, continuation) pair in one packed pass: a list of (sum_logprob, n_tokens, is_greedy).
        Neighbouring pairs that repeat a context compute it once.  An invalid pair fails the whole call with "pair <index>" in
        the message, before anything is computed."""
        n = len(pairs)
        ctx = [p[0].encode("utf-8") for p in pairs]
        cont = [p[1].encode("utf-8") for p in pairs]
        out = (_ffi.KjarniScoreResult * max(n, 1))()
        check_error(lib().kjarni_generator_score_batch(self._handle, (C.c_char_p * max(n, 1))(*ctx), (C.c_char_p * max(n, 1))(*cont), n, out))
        return [(float(out[i].sum_logprob), int(out[i].n_tokens), bool(out[i].is_greedy)) for i in range(n)]

    def score_tokens(self, context: str, continuation: str, top_k: int = 5):
        """score() token by token: (tokens u32 [n], logprobs f32 [n], top_tokens u32 [n, top_k], top_logprobs f32 [n, top_k])
        for the n tokens `continuation` adds; every row's alternatives most likely first (top_k 1 .. 8)."""
        r = _ffi.KjarniTokenScores()
        check_error(lib().kjarni_generator_score_tokens(self._handle, context.encode("utf-8"), continuation.encode("utf-8"), int(top_k),
                                                        C.byref(r)))
        try:
            n, k = int(r.n_tokens), int(r.top_k)
            return (np.ctypeslib.as_array(r.tokens, (n,)).copy(), np.ctypeslib.as_array(r.logprobs, (n,)).copy(),
                    np.ctypeslib.as_array(r.top_tokens, (n, k)).copy(), np.ctypeslib.as_array(r.top_logprobs, (n, k)).copy())
        finally:
            lib().kjarni_token_scores_free(C.byref(r))

    def generate_batch(self, prompts: Sequence[str], config: Optional[GenerationConfig] = None) -> List[str]:
        """generate() for every prompt, up to 8 of them (set_lanes) decoded in lock step; texts in prompt order."""
        arr = _ffi.KjarniStringArray()
        raw = [p.encode("utf-8") for p in prompts]
        ptrs = (C.c_char_p * max(len(raw), 1))(*raw)
        check_error(lib().kjarni_generator_generate_batch(self._handle, ptrs, len(raw), _gen(config), C.byref(arr)))
        try:
            return arr.to_list()
        finally:
            arr.free()

    def set_lanes(self, lanes: int):
        """Lanes generate_batch() runs with (1..8, 0 = 8)."""
        check_error(lib().kjarni_hip_generator_set_lanes(self._handle, lanes))

    def set_wide_lanes(self, lanes: int):
        """1..64: generate_batch() runs the decoder's generate_wide with that width (the wide step above 8 lanes, f32 / bf16
        safetensors checkpoints); 0 (the default) = off, the lanes path as set by set_lanes()."""
        check_error(lib().kjarni_hip_generator_set_wide_lanes(self._handle, lanes))

    def set_prompt_lookup(self, draft_tokens: int):
        """Prompt-lookup decoding for generate() / stream(): 0 = off (the default), 1..7 drafted tokens per step.  Applies to
        greedy configs without a repetition penalty or an n-gram ban; the text is the plain path's."""
        check_error(lib().kjarni_hip_generator_set_prompt_lookup(self._handle, draft_tokens))

    def set_prompt_lookup_sampling(self, on: bool):
        """Prompt-lookup decoding for sampled configs too, with or without a repetition penalty (off by default): taken when
        set_prompt_lookup() is 1..7 and the config has no n-gram ban; the text is the plain path's for the same seed."""
        check_error(lib().kjarni_hip_generator_set_prompt_lookup_sampling(self._handle, 1 if on else 0))

    def set_draft_model(self, model_dir_or_gguf: Optional[str], draft_tokens: int = 0):
        """A draft model for generate() / stream(): the checkpoint is loaded on this handle's device and owned by it, and
        proposes draft_tokens (1..7) tokens per verify step; None / 0 frees it.  While set it takes precedence over prompt
        lookup for greedy configs without processors and sampled configs without an n-gram ban; the text is the plain
        path's for the same seed."""
        path = model_dir_or_gguf.encode("utf-8") if model_dir_or_gguf else None
        check_error(lib().kjarni_hip_generator_set_draft_model(self._handle, path, int(draft_tokens)))

    def set_logprobs(self, top_k: Optional[int]):
        """Log-probabilities for every later request: top_k 0..8 alternatives per emitted token (0: the token's own logprob
        alone), None or -1 = off (the default).  While set, requests take the plain loop even when prompt lookup or a draft
        model is switched on.  The distribution is score()'s: the raw logits, before processors, temperature and the cut."""
        check_error(lib().kjarni_hip_generator_set_logprobs(self._handle, -1 if top_k is None else int(top_k)))

    def last_logprobs(self, prompt_index: int = 0):
        """(tokens u32 [n], logprobs f32 [n], top_tokens u32 [n, top_k], top_logprobs f32 [n, top_k]) of the tokens the last
        generate() / stream() call (prompt_index 0) or prompt `prompt_index` of the last generate_batch() emitted; empty arrays before any call and after one that ran with logprobs off."""
        r = _ffi.KjarniTokenScores()
        check_error(lib().kjarni_hip_generator_last_logprobs(self._handle, int(prompt_index), C.byref(r)))
        try:
            n, k = int(r.n_tokens), int(r.top_k)
            if n == 0:
                return (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros((0, k), np.uint32), np.zeros((0, k), np.float32))
            top = (np.ctypeslib.as_array(r.top_tokens, (n, k)).copy(), np.ctypeslib.as_array(r.top_logprobs, (n, k)).copy()) if k else \
                (np.zeros((n, 0), np.uint32), np.zeros((n, 0), np.float32))
            return (np.ctypeslib.as_array(r.tokens, (n,)).copy(), np.ctypeslib.as_array(r.logprobs, (n,)).copy()) + top
        finally:
            lib().kjarni_token_scores_free(C.byref(r))

    def set_constraint(self, pattern: Optional[str]):
        """Constrained decoding for generate() / stream(): every later request emits only text that `pattern` matches in full
        (kjarni_amd.constraints has builders: choices, integer, number, json_string, json_object); None restores the plain
        behaviour.  The token table comes from this handle's tokenizer, once per pattern.  While set, requests take the plain
        loop even when prompt lookup or a draft model is switched on; generate_batch() constrains every prompt of the batch on
        its lane (batch_constraint_result).  Nested or recursive JSON is a grammar: set_grammar."""
        check_error(lib().kjarni_hip_generator_set_constraint(self._handle, pattern.encode("utf-8") if pattern else None))

    def constraint_result(self):
        """How the last constrained request ended: final_state, device_state, accepted, complete, violated."""
        from .constraints import result_dict
        r = _ffi.KjarniHipConstraintResult()
        check_error(lib().kjarni_hip_generator_constraint_result(self._handle, C.byref(r)))
        return result_dict(r)

    def batch_constraint_result(self, prompt_index: int):
        """How prompt `prompt_index` of the last generate_batch() ended under the handle's pattern or grammar: kind (0 none, 1
        pattern, 2 grammar), final_state, final_depth, device_state, device_depth, accepted, complete, violated.  Zeros with
        kind 0 before a call, after an unconstrained one and for an index the call did not have."""
        from .constraints import lane_result_dict
        r = _ffi.KjarniHipLaneAutomatonResult()
        check_error(lib().kjarni_hip_generator_batch_constraint_result(self._handle, int(prompt_index), C.byref(r)))
        return lane_result_dict(r)

    def batch_seed(self, prompt_index: int) -> int:
        """Test hook: the seed of the generator prompt `prompt_index` of the last generate_batch() drew from; seed() with it and
        generate() of that prompt alone take the same draws."""
        return int(lib().kjarni_hip_generator_batch_seed(self._handle, int(prompt_index)))

    def set_grammar(self, rules):
        """Constrained decoding under a grammar: rules [(name, pattern)] as kjarni_amd.constraints.json_value / json_schema
        return them (rule 0 the start rule, patterns calling each other with (?&name)); None or [] removes it.  A handle holds a
        pattern or a grammar: setting one clears the other.  Requests take the plain loop as under set_constraint."""
        rules = list(rules or [])
        names = (C.c_char_p * max(len(rules), 1))(*[n.encode("utf-8") for n, _ in rules])
        pats = (C.c_char_p * max(len(rules), 1))(*[p.encode("utf-8") for _, p in rules])
        check_error(lib().kjarni_hip_generator_set_grammar(self._handle, names, pats, len(rules)))

    def grammar_result(self):
        """How the last request under a grammar ended: final_state, final_depth, device_state, device_depth, accepted, complete,
        violated."""
        from .constraints import grammar_result_dict
        r = _ffi.KjarniHipGrammarResult()
        check_error(lib().kjarni_hip_generator_grammar_result(self._handle, C.byref(r)))
        return grammar_result_dict(r)

    def set_prefix_reuse(self, on: bool):
        """Keep the cached rows of the tokens a call's prompt shares with the call before (off by default): score() over several
        continuations of one context prefills the context once, generate_batch() the prefix its prompts share."""
        check_error(lib().kjarni_hip_generator_set_prefix_reuse(self._handle, 1 if on else 0))

    def set_fp8_matrix_cores(self, on: bool):
        """FP8 checkpoints: multiply the codes themselves on the bf16 matrix cores in the prompt GEMM, and accept the checkpoint on
        more than 8 lanes (set_wide_lanes).  Off by default; a no-op on a checkpoint that is not FP8."""
        check_error(lib().kjarni_hip_generator_set_fp8_matrix_cores(self._handle, 1 if on else 0))

    def prefix_stats(self):
        """(reused, computed): prompt tokens whose cache rows were kept / computed by the calls that ran with reuse on."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        lib().kjarni_hip_generator_prefix_stats(self._handle, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def verify_gemv_calls(self):
        """(streamed, fallback) projections of prompt-lookup verify steps since load: moves only when a call took the lookup loop."""
        a, b = C.c_uint64(), C.c_uint64()
        lib().kjarni_hip_generator_verify_gemv_calls(self._handle, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def stream(self, prompt: str, on_token: Callable[[str], bool], config: Optional[GenerationConfig] = None, cancel=None):
        cb = _stream_cb(on_token)
        check_error(lib().kjarni_generator_stream(self._handle, prompt.encode("utf-8"), _gen(config), cb, None,
                                                  cancel._handle if cancel is not None else None))

    # ---- kjarni_hip.h hooks on a live handle ----
    def resolve(self, config: Optional[GenerationConfig] = None) -> ResolvedGeneration:
        r = _ffi.KjarniResolvedGeneration()
        check_error(lib().kjarni_hip_generator_resolve(self._handle, _gen(config), C.byref(r)))
        return _resolved(r)

    def encode(self, prompt: str, config: Optional[GenerationConfig] = None) -> List[int]:
        n = C.c_size_t()
        check_error(lib().kjarni_hip_generator_encode(self._handle, prompt.encode("utf-8"), _gen(config), None, 0, C.byref(n)))
        ids = np.zeros(max(n.value, 1), np.uint32)
        check_error(lib().kjarni_hip_generator_encode(self._handle, prompt.encode("utf-8"), _gen(config),
                                                      ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, C.byref(n)))
        return ids[: n.value].tolist()

    def seed(self, seed: int):
        lib().kjarni_hip_generator_seed(self._handle, seed)

    def set_device_sampling(self, on: bool):
        """Sampling / logits processors with the O(vocab) work on the device (default) or on a host copy of the logits."""
        lib().kjarni_hip_generator_set_device_sampling(self._handle, 1 if on else 0)
