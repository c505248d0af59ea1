"""Decoder embedders without a GPU: the new symbols are declared, exported and bound with their arity and answer NULL as
declared; the packing rule (kjarni_hip_embed_plan) against a Python restatement; the embedding entry of the BPE tokenizer
(add_special_tokens = true: the `single` template of a TemplateProcessing post-processor) on copies of the Qwen2 test
tokenizer with each supported post_processor shape."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi, decoder
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
L = kjarni_amd.lib()

SYMBOLS = {
    "kjarni_hip_decoder_embed": 6, "kjarni_hip_embed_plan": 11, "kjarni_hip_op_packed_causal_attention": 15, "kjarni_hip_op_rope": 11,
    "kjarni_hip_op_rope_rows": 11, "kjarni_hip_op_qk_norm_rope_rows": 18, "kjarni_hip_op_last_token_pool": 11,
    "kjarni_bpe_tokenizer_encode_embedding": 6,
}


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kjarni_hip.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/kjarni_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is C.c_int32
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name
    assert decoder.EMBED_CHUNK_ROWS == 2048 and "#define KJARNI_HIP_EMBED_CHUNK_ROWS 2048" in open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()


def test_null_handles_and_pointers():
    ids, off = (C.c_uint32 * 3)(5, 6, 7), (C.c_int32 * 2)(0, 3)
    out = (C.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    f4 = (C.c_float * 64)()
    i4 = (C.c_int32 * 4)(0, 1, 2, 3)
    n = C.c_int32(7)
    assert L.kjarni_hip_decoder_embed(None, ids, off, 1, 1, out) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_embed(None, None, None, 0, 1, None) == E.NULL_POINTER           # the handle comes first
    assert L.kjarni_hip_embed_plan(None, 1, 64, None, C.byref(n), None, 0, C.byref(n), None, 0, C.byref(n)) == E.NULL_POINTER
    assert L.kjarni_hip_embed_plan(i4, 1, 64, None, None, None, 0, C.byref(n), None, 0, C.byref(n)) == E.NULL_POINTER
    assert L.kjarni_hip_embed_plan(i4, 1, 64, None, C.byref(n), None, 0, None, None, 0, C.byref(n)) == E.NULL_POINTER
    assert L.kjarni_hip_embed_plan(i4, 1, 64, None, C.byref(n), None, 0, C.byref(n), None, 0, None) == E.NULL_POINTER
    assert n.value == 7
    A = L.kjarni_hip_op_packed_causal_attention
    assert A(0, None, 16, f4, 16, f4, 16, 1, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, None, 16, f4, 16, 1, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, None, 16, 1, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, f4, 16, 1, None, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, f4, 16, 1, i4, 1, 1, 1, 16, None, 16) == E.NULL_POINTER
    assert L.kjarni_hip_op_rope(0, None, 16, 1, 1, 1, 16, f4, f4, 1, 0) == E.NULL_POINTER
    assert L.kjarni_hip_op_rope(0, f4, 16, 1, 1, 1, 16, None, f4, 1, 0) == E.NULL_POINTER
    assert L.kjarni_hip_op_rope_rows(0, f4, 16, 1, 1, 1, 16, f4, f4, 1, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_rope_rows(0, None, 16, 1, 1, 1, 16, f4, f4, 1, i4) == E.NULL_POINTER
    Q = L.kjarni_hip_op_qk_norm_rope_rows
    assert Q(0, None, 16, 1, f4, 16, 1, 1, 1, 1, 16, f4, f4, 1e-6, f4, f4, 1, i4) == E.NULL_POINTER
    assert Q(0, f4, 16, 1, f4, 16, 1, 1, 1, 1, 16, f4, f4, 1e-6, f4, f4, 1, None) == E.NULL_POINTER
    assert Q(0, f4, 16, 1, f4, 16, 1, 1, 1, 1, 16, None, f4, 1e-6, f4, f4, 1, i4) == E.NULL_POINTER
    P = L.kjarni_hip_op_last_token_pool
    assert P(0, None, 16, 1, i4, 1, 16, f4, 1e-6, 1, out) == E.NULL_POINTER
    assert P(0, f4, 16, 1, None, 1, 16, f4, 1e-6, 1, out) == E.NULL_POINTER
    assert P(0, f4, 16, 1, i4, 1, 16, None, 1e-6, 1, out) == E.NULL_POINTER
    assert P(0, f4, 16, 1, i4, 1, 16, f4, 1e-6, 1, None) == E.NULL_POINTER
    cnt = C.c_size_t(7)
    assert L.kjarni_bpe_tokenizer_encode_embedding(None, b"a", 0, ids, 3, C.byref(cnt)) == E.NULL_POINTER
    assert cnt.value == 7 and list(out) == [9.0] * 4 and list(ids) == [5, 6, 7]                  # nothing written


# ---- the packing rule ---------------------------------------------------------------------------------------------------------

def _plan(lengths, head_dim):
    """The rule, restated: (chunk_first_seq, vec blocks, mfma blocks)."""
    first, vec, mfma = [], [], []
    rows = 0
    for i, n in enumerate(lengths):
        if not first or rows + n > 2048:
            first.append(i)
            rows = 0
        c = len(first) - 1
        if n >= 256 and head_dim in (64, 128):
            mfma += [(c, rows, q0, n) for q0 in range(0, n, 128)]
        else:
            vec += [(c, rows, q0, n) for q0 in range(0, n, 32)]
        rows += n
    return first + [len(lengths)], vec, mfma


PLAN_LENGTHS = [[1], [2048], [2047, 2], [1000, 1000, 1000], [31, 32, 33, 255, 256, 257],
                np.random.default_rng(11).integers(1, 201, 300).tolist()]


@pytest.mark.parametrize("lengths", PLAN_LENGTHS, ids=lambda x: f"n{len(x)}-sum{sum(x)}")
@pytest.mark.parametrize("head_dim", [32, 64, 128])
def test_embed_plan(lengths, head_dim):
    first, vec, mfma = decoder.embed_plan(lengths, head_dim)
    want_first, want_vec, want_mfma = _plan(lengths, head_dim)
    assert first.tolist() == want_first
    assert [tuple(b) for b in vec.tolist()] == want_vec and [tuple(b) for b in mfma.tolist()] == want_mfma
    # chunk boundaries: at most 2 048 rows each, nothing straddles, greedy (the next sequence would not have fitted)
    assert first[0] == 0 and first[-1] == len(lengths) and (np.diff(first) > 0).all()
    for c in range(len(first) - 1):
        rows = sum(lengths[first[c]:first[c + 1]])
        assert rows <= 2048
        if c + 2 < len(first):
            assert rows + lengths[first[c + 1]] > 2048
    # every query block exactly once, in the right route's table, inside its own sequence
    seen = {}
    for route, table, step in (("vec", vec, 32), ("mfma", mfma, 128)):
        for c, start, q0, n in table.tolist():
            assert q0 % step == 0 and 0 <= q0 < n and start + n <= 2048
            assert (n >= 256 and head_dim in (64, 128)) == (route == "mfma")
            key = (c, start, q0)
            assert key not in seen
            seen[key] = n
    want = set()
    for c in range(len(first) - 1):
        start = 0
        for n in lengths[first[c]:first[c + 1]]:
            step = 128 if (n >= 256 and head_dim in (64, 128)) else 32
            want |= {(c, start, q0) for q0 in range(0, n, step)}
            start += n
    assert set(seen) == want


def test_embed_plan_refuses_what_no_chunk_holds():
    for bad, at in (([2049], 0), ([5, 0, 3], 1), ([7, -1], 1)):
        with pytest.raises(KjarniException) as e:
            decoder.embed_plan(bad)
        assert e.value.code == E.INVALID_CONFIG and f"lengths[{at}]" in str(e.value)
    first, vec, mfma = decoder.embed_plan([])
    assert first.tolist() == [0] and len(vec) == 0 and len(mfma) == 0


def test_embed_plan_counts_without_buffers():
    a = (C.c_int32 * 3)(300, 40, 2000)
    nc, nv, nm = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.kjarni_hip_embed_plan(a, 3, 64, None, C.byref(nc), None, 0, C.byref(nv), None, 0, C.byref(nm)) == E.OK
    assert (nc.value, nv.value, nm.value) == (2, 2, 3 + 16)


# ---- the embedding entry of the tokenizer -----------------------------------------------------------------------------------------

EOT, IM_START = "<|endoftext|>", "<|im_start|>"     # ids 700 and 701 of tests/golden/bpe_qwen2_tokenizer.json


def _special(name, ident):
    return {name: {"id": name, "ids": [ident], "tokens": [name]}}


def _template(single, specials):
    pieces = [{"Sequence": {"id": "A", "type_id": 0}} if p == "$A" else {"SpecialToken": {"id": p, "type_id": 0}} for p in single]
    pair = pieces + [{"Sequence": {"id": "B", "type_id": 1}}]
    return {"type": "TemplateProcessing", "single": pieces, "pair": pair, "special_tokens": specials}


BYTE_LEVEL = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": False, "use_regex": False}
POST_PROCESSORS = {
    "none": (None, [], []),
    "bytelevel": (BYTE_LEVEL, [], []),
    "append": (_template(["$A", EOT], _special(EOT, 700)), [], [700]),
    "prepend": (_template([IM_START, "$A"], _special(IM_START, 701)), [701], []),
    "sequence": ({"type": "Sequence", "processors": [BYTE_LEVEL, _template([IM_START, "$A", EOT], {**_special(IM_START, 701), **_special(EOT, 700)})]},
                 [701], [700]),
}
TEXTS = ["Hello world", "", "  two  spaces and a newline\n", "café naïve 你好", "x" * 40 + " " + EOT + " tail"]


def _tokenizer(tmp_path, post_processor):
    from kjarni_amd.chat import BpeTokenizer
    j = json.load(open(os.path.join(GOLDEN, "bpe_qwen2_tokenizer.json")))
    j["post_processor"] = post_processor
    p = str(tmp_path / "tokenizer.json")
    with open(p, "w") as f:
        json.dump(j, f)
    return BpeTokenizer(p)


@pytest.mark.parametrize("kind", sorted(POST_PROCESSORS))
def test_embedding_entry_frames_the_plain_ids(tmp_path, kind):
    pp, before, after = POST_PROCESSORS[kind]
    tok = _tokenizer(tmp_path, pp)
    for text in TEXTS:
        plain = tok.encode(text)
        assert tok.encode_embedding(text) == before + plain + after, (kind, text)
        assert tok.encode(text) == plain                                    # the existing entry adds nothing
    # truncation from the right: the text's own tokens are cut, the framing survives, the framed length respects max_length
    text = TEXTS[2] + TEXTS[3]
    plain, frame = tok.encode(text), len(before) + len(after)
    assert len(plain) > 8
    for max_length in (len(plain) + frame + 5, len(plain) + frame, len(plain) + frame - 1, frame + 3, frame + 1, max(frame, 1)):
        got = tok.encode_embedding(text, max_length)
        keep = min(len(plain), max_length - frame)
        assert got == before + plain[:keep] + after and len(got) <= max_length, (kind, max_length)
    if frame == 2:                                                          # a limit below the framing: the framing still survives
        assert tok.encode_embedding(text, 1) == before + after


def test_embedding_entry_with_ids_from_the_vocabulary(tmp_path):
    """A special token whose ids the template does not list is looked up by its name."""
    pp = _template(["$A", EOT], {})
    assert _tokenizer(tmp_path, pp).encode_embedding("Hello") == _tokenizer(tmp_path, None).encode("Hello") + [700]


@pytest.mark.parametrize("pp,name", [({"type": "RobertaProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0]}, "RobertaProcessing"),
                                     ({"type": "BertProcessing", "sep": ["[SEP]", 2], "cls": ["[CLS]", 0]}, "BertProcessing"),
                                     ({"type": "Sequence", "processors": [BYTE_LEVEL, {"type": "RobertaProcessing"}]}, "RobertaProcessing")])
def test_embedding_entry_refuses_other_post_processors_by_name(tmp_path, pp, name):
    tok = _tokenizer(tmp_path, pp)
    assert tok.encode("Hello") == _tokenizer(tmp_path, None).encode("Hello")       # the generation entry never reads it
    with pytest.raises(KjarniException) as e:
        tok.encode_embedding("Hello")
    assert e.value.code == E.INVALID_CONFIG and f"unsupported post_processor '{name}'" in str(e.value)


def test_registry_names_of_the_decoder_embedders(tmp_path):
    """The names resolve (to a directory that is not there: MODEL_NOT_FOUND naming it), as do the lower-cased repo ids."""
    for name, repo in (("qwen3-embedding-0.6b", "Qwen_Qwen3-Embedding-0.6B"), ("Qwen/Qwen3-Embedding-4B", "Qwen_Qwen3-Embedding-4B"),
                       ("qwen/qwen3-embedding-8b", "Qwen_Qwen3-Embedding-8B")):
        with pytest.raises(KjarniException) as e:
            kjarni_amd.Embedder(name, cache_dir=str(tmp_path))
        assert e.value.code == E.MODEL_NOT_FOUND and "is not downloaded" in str(e.value) and repo in str(e.value), str(e.value)
