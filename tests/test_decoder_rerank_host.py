"""Decoder rerankers without a GPU: the new symbols are declared, exported and bound with their arity and answer NULL as declared;
the answer plan (kjarni_hip_answer_plan) against a Python restatement of its rule, case by case and on random batches; the
prompt rule (kjarni_hip_rerank_prompt_ids) on a tokenizer written here; the registry names."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException
from tests import rerank_fixture as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {
    "kjarni_hip_decoder_answer_logits": 7, "kjarni_hip_decoder_answer_rows": 3, "kjarni_hip_answer_plan": 23, "kjarni_hip_op_answer_logits": 16,
    "kjarni_reranker_set_instruction": 2, "kjarni_hip_rerank_prompt_ids": 8, "kjarni_hip_reranker_answer_rows": 3,
}


def _declarations():
    text = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("kjarni_hip.h", "kjarni.h"))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(kjarni_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_symbols_are_declared_exported_and_bound_with_their_arity():
    decl = _declarations()
    for name, arity in SYMBOLS.items():
        assert name in decl, f"{name} is not declared in include/"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is (None if name.endswith("_rows") else C.c_int32)
        assert len(argtypes) == arity == len([a for a in decl[name].split(",") if a.strip()]), name
    for attr in ("answer_logits", "answer_logits_flat", "answer_rows"):
        assert hasattr(kjarni_amd.HipDecoder, attr)
    for attr in ("set_instruction", "answer_rows"):
        assert hasattr(kjarni_amd.Reranker, attr)
    from kjarni_amd import decoder, ops
    assert callable(ops.answer_logits) and callable(ops.answer_plan) and callable(kjarni_amd.answer_plan)
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    assert f"#define KJARNI_HIP_ANSWER_MAX_TARGETS {decoder.ANSWER_MAX_TARGETS}\n" in header and decoder.ANSWER_MAX_TARGETS == 8


def test_null_handles_and_pointers(tmp_path):
    ids, off, tg = (C.c_uint32 * 3)(5, 6, 7), (C.c_int32 * 2)(0, 3), (C.c_uint32 * 2)(1, 2)
    out = (C.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    assert L.kjarni_hip_decoder_answer_logits(None, ids, off, 1, tg, 2, out) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_answer_logits(None, None, None, 0, None, 0, None) == E.NULL_POINTER      # the handle comes first
    a, b = C.c_uint64(7), C.c_uint64(7)
    L.kjarni_hip_decoder_answer_rows(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    L.kjarni_hip_decoder_answer_rows(None, None, None)
    a, b = C.c_uint64(7), C.c_uint64(7)
    L.kjarni_hip_reranker_answer_rows(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    L.kjarni_hip_reranker_answer_rows(None, None, None)
    n = [C.c_int32(7) for _ in range(6)]
    r = [C.byref(x) for x in n]

    def plan(ids_, off_, counts):
        c = counts
        return L.kjarni_hip_answer_plan(ids_, off_, 1, 64, 1, None, None, c[0], None, 0, c[1], None, 0, c[2], None, 0, c[3], None, 0, c[4],
                                        None, 0, c[5])
    assert plan(None, off, r) == E.NULL_POINTER and plan(ids, None, r) == E.NULL_POINTER
    for missing in range(6):
        assert plan(ids, off, [None if i == missing else r[i] for i in range(6)]) == E.NULL_POINTER
    assert [x.value for x in n] == [7] * 6
    assert plan(ids, off, r) == E.OK and [x.value for x in n] == [1, 0, 1, 0, 0, 1]                         # counts without tables
    f4, i4 = (C.c_float * 64)(), (C.c_int32 * 4)(0, 1, 2, 3)
    A = L.kjarni_hip_op_answer_logits
    assert A(0, None, 16, 1, i4, 1, 16, f4, None, 1e-6, f4, 4, 0, tg, 2, out) == E.NULL_POINTER
    assert A(0, f4, 16, 1, None, 1, 16, f4, None, 1e-6, f4, 4, 0, tg, 2, out) == E.NULL_POINTER
    assert A(0, f4, 16, 1, i4, 1, 16, None, None, 1e-6, f4, 4, 0, tg, 2, out) == E.NULL_POINTER
    assert A(0, f4, 16, 1, i4, 1, 16, f4, None, 1e-6, None, 4, 0, tg, 2, out) == E.NULL_POINTER
    assert A(0, f4, 16, 1, i4, 1, 16, f4, None, 1e-6, f4, 4, 0, None, 2, out) == E.NULL_POINTER
    assert A(0, f4, 16, 1, i4, 1, 16, f4, None, 1e-6, f4, 4, 0, tg, 2, None) == E.NULL_POINTER
    assert L.kjarni_reranker_set_instruction(None, b"x") == E.NULL_POINTER and L.kjarni_reranker_set_instruction(None, None) == E.NULL_POINTER
    P = L.kjarni_hip_rerank_prompt_ids
    tok = RF.write_tokenizer(str(tmp_path / "tokenizer.json")).encode()
    cnt = C.c_size_t(7)
    assert P(None, None, b"q", b"d", 64, ids, 3, C.byref(cnt)) == E.NULL_POINTER
    assert P(tok, None, None, b"d", 64, ids, 3, C.byref(cnt)) == E.NULL_POINTER
    assert P(tok, None, b"q", None, 64, ids, 3, C.byref(cnt)) == E.NULL_POINTER
    assert P(tok, None, b"q", b"d", 64, ids, 3, None) == E.NULL_POINTER
    assert P(tok, None, b"q", b"d", 64, None, 3, C.byref(cnt)) == E.NULL_POINTER
    assert P(tok, b"\xff", b"q", b"d", 64, ids, 3, C.byref(cnt)) == E.INVALID_UTF8
    assert cnt.value == 7 and list(out) == [9.0] * 4 and list(ids) == [5, 6, 7]                              # nothing written
    assert P(tok, None, b"q", b"d", 4096, None, 0, C.byref(cnt)) == E.OK and cnt.value > 7                   # the count without a buffer


# ---- the plan -------------------------------------------------------------------------------------------------------------------

def _lcp(a, b):
    k = 0
    while k < min(len(a), len(b)) and a[k] == b[k]:
        k += 1
    return k


def _plan(seqs, head_dim, min_shared):
    """The rule of the issue, restated: score_plan's grouping with firsts[b] = len_b - 1; the gather table lists the row of every
    sequence's last token."""
    B = len(seqs)
    lens = [len(s) for s in seqs]
    units, i = [], 0
    while i < B:
        p, j = lens[i] - 1, i + 1
        while j < B:
            q = min(p, lens[j] - 1, _lcp(seqs[i], seqs[j]))
            if q < min_shared or q + sum(lens[t] - q for t in range(i, j + 1)) > 2048 or max(lens[t] - q for t in range(i, j + 1)) >= 256:
                break
            p, j = q, j + 1
        units.append((i, j, p) if j - i >= 2 else (i, i + 1, 0))
        i = units[-1][1]
    chunks, groups, vec, mfma, pre, gather = [], [], [], [], [], []

    def blocks(c, start, n):
        if n >= 256 and head_dim in (64, 128):
            mfma.extend((c, start, q0, n) for q0 in range(0, n, 128))
        else:
            vec.extend((c, start, q0, n) for q0 in range(0, n, 32))
    for i, j, p in units:
        cost = p + sum(lens[t] - p for t in range(i, j))
        if not chunks or chunks[-1][1] + cost > 2048:
            chunks.append([i, 0])
        c, row = len(chunks) - 1, chunks[-1][1]
        pf = row
        if j - i >= 2:
            groups.append((c, i, j - i, p))
            blocks(c, row, p)
            row += p
        for t in range(i, j):
            own = lens[t] - p
            if j - i >= 2:
                pre.extend((c, row, q0, own, pf, p) for q0 in range(0, own, 32))
            else:
                blocks(c, row, own)
            gather.append((c, row + own - 1, t))
            row += own
        chunks[-1][1] = row
    return {"chunk_first_seq": [c[0] for c in chunks] + [B], "chunk_rows": [c[1] for c in chunks], "groups": groups, "vec": vec, "mfma": mfma,
            "prefix": pre, "gather": gather}


def _docs(spec, seed=3, vocab=1000):
    """spec: (query key, query length, document length) per sequence; equal keys share the query's tokens and every document starts
    with a token of its own, so that the common prefix of two sharers is exactly the query."""
    rng = np.random.default_rng(seed)
    ctx, out = {}, []
    for n, (key, qlen, dlen) in enumerate(spec):
        if key not in ctx:
            ctx[key] = [vocab + 10 * len(ctx)] + rng.integers(0, vocab, qlen - 1).tolist()
        out.append(ctx[key][:qlen] + [2000 + n] + rng.integers(0, vocab, dlen - 1).tolist())
    return out


_SAME = [5, 6, 7, 8, 9]
CASES = {
    "nothing_shared": (_docs([("a", 5, 3), ("b", 7, 2), ("c", 3, 9)]), 64, 2),
    "one_query_six_documents": (_docs([("a", 20, n) for n in (3, 40, 7, 12, 1, 25)]), 64, 2),
    "two_identical_sequences": ([list(_SAME), list(_SAME)], 64, 2),
    "a_prefix_of_the_next": ([[5, 6, 7], [5, 6, 7, 8, 9], [5, 6, 7, 8, 9, 10]], 64, 2),
    "interleaved_queries": (_docs([("a", 20, 4), ("b", 20, 4), ("a", 20, 6), ("b", 20, 6)]), 64, 2),
    "remainder_of_256_ends_the_group": (_docs([("a", 20, 10), ("a", 20, 255), ("a", 20, 256), ("a", 20, 5)]), 64, 2),
    "remainders_of_256_and_more": (_docs([("a", 20, 256), ("a", 20, 300), ("a", 20, 256)]), 64, 2),
    "group_split_by_the_chunk": (_docs([("a", 100, 250)] * 9), 64, 2),
    "mfma_prefix": (_docs([("a", 300, 5), ("a", 300, 40), ("a", 300, 12)]), 64, 2),
    "twenty_of_120": (_docs([(n, 100, 20) for n in range(20)]), 64, 2),
}


def _check(seqs, head_dim, min_shared, what):
    got = kjarni_amd.answer_plan(seqs, head_dim, min_shared)
    want = _plan(seqs, head_dim, min_shared)
    for key in want:
        assert [tuple(r) if isinstance(r, list) else r for r in got[key].tolist()] == want[key], (what, key)
    lens = [len(s) for s in seqs]
    groups = [tuple(g) for g in got["groups"].tolist()]
    # the last token is never in a prefix: every group's prefix is shorter than every member
    for c, first, members, p in groups:
        assert all(p <= lens[t] - 1 for t in range(first, first + members)) and p >= min_shared, what
    # the gather row is the row of the last token: rebuild every chunk's row -> (sequence, position) map from the tables
    assert got["gather"][:, 2].tolist() == list(range(len(seqs))), what
    owner = {}
    for c, start, q0, n in got["vec"].tolist() + got["mfma"].tolist():
        owner.setdefault((c, start), n)                                          # a plain sequence, or a prefix
    rem = {(c, start): (n, pf, p) for c, start, q0, n, pf, p in got["prefix"].tolist()}
    for c, row, t in got["gather"].tolist():
        inside = [(s, n) for (cc, s), n in owner.items() if cc == c and s <= row < s + n] + \
                 [(s, n) for (cc, s), (n, pf, p) in rem.items() if cc == c and s <= row < s + n]
        assert len(inside) == 1 and row == inside[0][0] + inside[0][1] - 1, (what, t)          # the last row of its own block of rows
        if (c, inside[0][0]) in rem:
            n, pf, p = rem[(c, inside[0][0])]
            assert p + n == lens[t] and seqs[t][:p] == seqs[[g for g in groups if g[0] == c and g[1] <= t < g[1] + g[2]][0][1]][:p], (what, t)
        else:
            assert inside[0][1] == lens[t], (what, t)
    assert (got["chunk_rows"] <= 2048).all(), what
    saved = sum((m - 1) * p for _, _, m, p in groups)
    assert int(got["chunk_rows"].sum()) == sum(lens) - saved, what
    return got, groups


@pytest.mark.parametrize("name", sorted(CASES))
def test_answer_plan_matches_the_rule(name):
    seqs, head_dim, min_shared = CASES[name]
    got, groups = _check(seqs, head_dim, min_shared, name)
    if name == "nothing_shared":
        assert groups == [] and len(got["prefix"]) == 0
    if name == "one_query_six_documents":
        assert groups == [(0, 0, 6, 20)] and got["chunk_rows"].tolist() == [20 + 3 + 40 + 7 + 12 + 1 + 25]
    if name == "two_identical_sequences":
        assert groups == [(0, 0, 2, 4)] and got["gather"].tolist() == [[0, 4, 0], [0, 5, 1]]       # 4 shared rows, then one row each
    if name == "a_prefix_of_the_next":
        # [5, 6, 7] lends its first two tokens only -- its last token stays its own -- and takes the group's prefix down to 2
        assert groups == [(0, 0, 3, 2)] and got["gather"].tolist() == [[0, 2, 0], [0, 5, 1], [0, 9, 2]]
    if name == "interleaved_queries":
        assert groups == []
    if name == "remainder_of_256_ends_the_group":
        assert groups == [(0, 0, 2, 20)]
    if name == "remainders_of_256_and_more":
        assert groups == []
    if name == "group_split_by_the_chunk":
        assert groups == [(0, 0, 7, 100), (1, 7, 2, 100)] and got["chunk_rows"].tolist() == [100 + 7 * 250, 100 + 2 * 250]
    if name == "mfma_prefix":
        assert [tuple(b) for b in got["mfma"].tolist()] == [(0, 0, 0, 300), (0, 0, 128, 300), (0, 0, 256, 300)] and len(got["vec"]) == 0
    if name == "twenty_of_120":
        assert groups == [] and got["chunk_first_seq"].tolist() == [0, 17, 20] and got["chunk_rows"].tolist() == [17 * 120, 3 * 120]


def test_answer_plan_on_random_batches():
    rng = np.random.default_rng(11)
    for trial in range(20):
        spec = []
        for _ in range(int(rng.integers(1, 40))):
            key, qlen = int(rng.integers(0, 6)), int(rng.integers(1, 60))
            spec += [(key * 100 + qlen, qlen, int(rng.integers(1, 300))) for _ in range(int(rng.integers(1, 5)))]
        seqs = _docs(spec, seed=trial)
        if trial % 4 == 0:                                  # repeats and prefixes of the neighbour among them
            seqs = [s for s in seqs for _ in range(2)]
            seqs[1::4] = [s[:max(2, len(s) // 2)] for s in seqs[1::4]]
        for head_dim, min_shared in ((64, 2), (32, 8), (128, 1)):
            _check(seqs, head_dim, min_shared, trial)


def test_answer_plan_is_score_plan_at_the_last_token():
    """Built on score_plan: same chunks, groups and block tables as score_plan with firsts = len - 1."""
    seqs = CASES["one_query_six_documents"][0] + CASES["a_prefix_of_the_next"][0] + CASES["mfma_prefix"][0]
    a = kjarni_amd.answer_plan(seqs, 64, 2)
    s = kjarni_amd.score_plan(seqs, [len(x) - 1 for x in seqs], 64, 2)
    for key in ("chunk_first_seq", "chunk_rows", "groups", "vec", "mfma", "prefix"):
        assert a[key].tolist() == s[key].tolist(), key
    assert len(a["gather"]) == len(s["gather"]) == len(seqs)


def test_answer_plan_refusals():
    for seqs, words in (([[1]], "fewer than 2"), ([[1, 2], [3]], "(sequence 1)"), ([[1, 2], list(range(2049))], "(sequence 1)")):
        with pytest.raises(KjarniException) as e:
            kjarni_amd.answer_plan(seqs)
        assert e.value.code == E.INVALID_CONFIG and words in str(e.value), str(e.value)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.answer_plan([[1, 2]], min_shared=0)
    assert e.value.code == E.INVALID_CONFIG and "min_shared" in str(e.value)
    ids, off = (C.c_uint32 * 4)(1, 2, 3, 4), (C.c_int32 * 3)(0, 3, 1)
    n = [C.c_int32() for _ in range(6)]
    rc = L.kjarni_hip_answer_plan(ids, off, 2, 64, 1, None, None, C.byref(n[0]), None, 0, C.byref(n[1]), None, 0, C.byref(n[2]), None, 0,
                                  C.byref(n[3]), None, 0, C.byref(n[4]), None, 0, C.byref(n[5]))
    assert rc == E.INVALID_CONFIG and "offsets must not decrease" in _ffi.last_error()
    empty = kjarni_amd.answer_plan([])
    assert empty["chunk_first_seq"].tolist() == [0] and all(len(empty[k]) == 0 for k in ("groups", "vec", "mfma", "prefix", "gather"))


# ---- the prompt -----------------------------------------------------------------------------------------------------------------

def test_prompt_is_head_body_tail_encoded_alone(tmp_path):
    from kjarni_amd.chat import BpeTokenizer
    from kjarni_amd.reranker import rerank_prompt_ids
    path = RF.write_tokenizer(str(tmp_path / "tokenizer.json"))
    tok = BpeTokenizer(path)
    assert tok.encode("yes") == [RF.YES] and tok.encode("no") == [RF.NO]
    head, tail = tok.encode(RF.HEAD), tok.encode(RF.TAIL)
    assert head[0] == 701 and 702 in head and tail[0] == 702 and RF.THINK in tail and RF.END_THINK in tail   # added tokens are recognised
    for instruction in (None, "Find the passage that names the capital"):
        for query, doc in (("What is the capital of France?", "Paris is the capital of France."), ("a", ""), ("naïve café 你好", "x\n<Document>: y")):
            body = tok.encode(RF.body(query, doc, instruction))
            got = rerank_prompt_ids(path, query, doc, instruction, 4096)
            assert got == head + body + tail, (instruction, query)
            assert got[0] != 700 and got[-1] != 700                                                             # no BOS / EOS is added
    assert rerank_prompt_ids(path, "q", "d", None, 4096) == rerank_prompt_ids(path, "q", "d", RF.INSTRUCTION, 4096)


def test_prompt_cuts_the_document_from_the_right_and_refuses_to_cut_the_query(tmp_path):
    from kjarni_amd.chat import BpeTokenizer
    from kjarni_amd.reranker import rerank_prompt_ids
    path = RF.write_tokenizer(str(tmp_path / "tokenizer.json"))
    tok = BpeTokenizer(path)
    head, tail = tok.encode(RF.HEAD), tok.encode(RF.TAIL)
    query, doc = "Which river runs through Paris?", "The Seine runs through Paris. " * 6
    body, front = tok.encode(RF.body(query, doc)), tok.encode(RF.body(query, None)[:-len("\n<Document>: ")])
    frame = len(head) + len(tail)
    assert len(body) > len(front) + 20
    for limit in (frame + len(body) + 3, frame + len(body), frame + len(body) - 1, frame + len(front) + 5, frame + len(front)):
        got = rerank_prompt_ids(path, query, doc, None, limit)
        keep = min(len(body), limit - frame)
        assert got == head + body[:keep] + tail and len(got) <= limit, limit
    for limit in (frame + len(front) - 1, frame, 1):
        with pytest.raises(KjarniException) as e:
            rerank_prompt_ids(path, query, doc, None, limit)
        assert e.value.code == E.INVALID_CONFIG and "reach into the query" in str(e.value), str(e.value)
    # a prompt that fits is never refused, however small the room behind it
    assert rerank_prompt_ids(path, query, "", None, frame + len(tok.encode(RF.body(query, "")))) == head + tok.encode(RF.body(query, "")) + tail


def test_a_tokenizer_without_a_one_token_yes_is_a_load_error_that_names_it(tmp_path):
    from kjarni_amd.reranker import rerank_prompt_ids
    golden = os.path.join(ROOT, "tests", "golden", "bpe_qwen2_tokenizer.json")
    with pytest.raises(KjarniException) as e:
        rerank_prompt_ids(golden, "q", "d")
    assert e.value.code == E.LOAD_FAILED and '"yes"' in str(e.value) and "one token" in str(e.value), str(e.value)
    path = RF.write_tokenizer(str(tmp_path / "tokenizer.json"), words=("yes", "<think>", "</think>"))      # "no" is missing
    with pytest.raises(KjarniException) as e:
        rerank_prompt_ids(path, "q", "d")
    assert e.value.code == E.LOAD_FAILED and '"no"' in str(e.value), str(e.value)
    with pytest.raises(KjarniException) as e:
        rerank_prompt_ids(str(tmp_path / "missing.json"), "q", "d")
    assert e.value.code == E.LOAD_FAILED


# ---- the registry ---------------------------------------------------------------------------------------------------------------

def test_registry_names_of_the_decoder_rerankers(tmp_path):
    """The names resolve with the reranking task and the decoder architecture: the Reranker looks for their directory
    (MODEL_NOT_FOUND naming it, the embedder's wording), the Embedder refuses them as it refuses any other task's model."""
    for name, repo in (("qwen3-reranker-0.6b", "Qwen_Qwen3-Reranker-0.6B"), ("Qwen/Qwen3-Reranker-4B", "Qwen_Qwen3-Reranker-4B"),
                       ("qwen/qwen3-reranker-8b", "Qwen_Qwen3-Reranker-8B"), ("qwen3-reranker-8b", "Qwen_Qwen3-Reranker-8B"),
                       ("QWEN/QWEN3-RERANKER-0.6B", "Qwen_Qwen3-Reranker-0.6B")):
        with pytest.raises(KjarniException) as e:
            kjarni_amd.Reranker(name, cache_dir=str(tmp_path))
        msg = str(e.value)
        assert e.value.code == E.MODEL_NOT_FOUND and "is not downloaded (expected config.json, tokenizer.json and model.safetensors in" in msg
        assert repo in msg and "this build never downloads models" in msg, msg
        with pytest.raises(KjarniException) as e:
            kjarni_amd.Embedder(name, cache_dir=str(tmp_path))
        assert e.value.code != E.MODEL_NOT_FOUND and "not compatible" in str(e.value), str(e.value)
    # an embedder name is no reranker, and an encoder name behaves as before
    with pytest.raises(KjarniException) as e:
        kjarni_amd.Reranker("qwen3-embedding-0.6b", cache_dir=str(tmp_path))
    assert "not compatible" in str(e.value)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.Reranker("minilm-l6-v2-cross-encoder", cache_dir=str(tmp_path))
    assert e.value.code == E.MODEL_NOT_FOUND and "cross-encoder_ms-marco-MiniLM-L-6-v2" in str(e.value)
    # the new names resolve, yet stay out of the "Did you mean" lists: a substring of them alone suggests nothing new, and the
    # similarity list of a near miss is what it was
    for name, want in (("qwen3-reranker", "Unknown model 'qwen3-reranker'. Did you mean: qwen3-0.6b, qwen3-1.7b, qwen3-4b?"),
                       ("qwen3", "Unknown model 'qwen3'. Did you mean: qwen3-0.6b, qwen3-1.7b, qwen3-4b, qwen3-8b?"),
                       ("reranker-0.6b", None)):
        with pytest.raises(KjarniException) as e:
            kjarni_amd.Reranker(name, cache_dir=str(tmp_path))
        assert e.value.code == E.MODEL_NOT_FOUND and "reranker-" not in str(e.value).split("Did you mean")[-1].replace(name, ""), str(e.value)
        if want:
            assert str(e.value).endswith(want), str(e.value)
