"""Batched scoring without a GPU: the new symbols are declared, exported and bound with their arity and answer NULL as declared;
the plan (kjarni_hip_score_plan) against a Python restatement of its rule, case by case, and one gather table written out by
hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd._ffi import KjarniError as E
from kjarni_amd._ffi import KjarniException

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = kjarni_amd.lib()

SYMBOLS = {
    "kjarni_hip_decoder_score_batch": 9, "kjarni_hip_decoder_score_batch_rows": 3, "kjarni_hip_score_plan": 24,
    "kjarni_hip_op_packed_prefix_attention": 15, "kjarni_hip_op_score_gather_norm": 12, "kjarni_generator_score_batch": 5,
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
    for attr in ("score_batch", "score_batch_flat", "score_batch_rows"):
        assert hasattr(kjarni_amd.HipDecoder, attr)
    assert hasattr(kjarni_amd.Generator, "score_batch") and callable(kjarni_amd.score_plan)
    from kjarni_amd import decoder, ops
    assert callable(ops.packed_prefix_attention) and callable(ops.score_gather_norm)
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    assert f"#define KJARNI_HIP_SCORE_MIN_SHARED {decoder.SCORE_MIN_SHARED} " in header and decoder.SCORE_MIN_SHARED >= 1
    source = open(os.path.join(ROOT, "kjarni_amd", "csrc", "llm.h")).read()
    assert "kScoreMinShared = KJARNI_HIP_SCORE_MIN_SHARED;" in source and f"#define KJARNI_HIP_SCORE_MIN_SHARED {decoder.SCORE_MIN_SHARED} " in source


def test_null_handles_and_pointers():
    ids, off, fs = (C.c_uint32 * 3)(5, 6, 7), (C.c_int32 * 2)(0, 3), (C.c_int32 * 1)(1)
    lp = (C.c_float * 4)(9.0, 9.0, 9.0, 9.0)
    top = (C.c_uint32 * 4)(9, 9, 9, 9)
    f4 = (C.c_float * 64)()
    i4 = (C.c_int32 * 4)(0, 1, 2, 3)
    assert L.kjarni_hip_decoder_score_batch(None, ids, off, 1, fs, 1, lp, top, lp) == E.NULL_POINTER
    assert L.kjarni_hip_decoder_score_batch(None, None, None, 0, None, 1, None, None, None) == E.NULL_POINTER    # the handle comes first
    a, b = C.c_uint64(7), C.c_uint64(7)
    L.kjarni_hip_decoder_score_batch_rows(None, C.byref(a), C.byref(b))
    assert (a.value, b.value) == (0, 0)
    L.kjarni_hip_decoder_score_batch_rows(None, None, None)
    n = [C.c_int32(7) for _ in range(6)]
    r = [C.byref(x) for x in n]

    def plan(ids_, off_, fs_, counts):
        c = counts
        return L.kjarni_hip_score_plan(ids_, off_, fs_, 1, 64, 1, None, None, c[0], None, 0, c[1], None, 0, c[2], None, 0, c[3], None, 0, c[4],
                                       None, 0, c[5])
    assert plan(None, off, fs, r) == E.NULL_POINTER and plan(ids, None, fs, r) == E.NULL_POINTER and plan(ids, off, None, r) == E.NULL_POINTER
    for missing in range(6):
        assert plan(ids, off, fs, [None if i == missing else r[i] for i in range(6)]) == E.NULL_POINTER
    assert [x.value for x in n] == [7] * 6
    assert plan(ids, off, fs, r) == E.OK and [x.value for x in n] == [1, 0, 1, 0, 0, 2]                             # counts without tables
    A = L.kjarni_hip_op_packed_prefix_attention
    assert A(0, None, 16, f4, 16, f4, 16, 2, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, None, 16, f4, 16, 2, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, None, 16, 2, i4, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, f4, 16, 2, None, 1, 1, 1, 16, f4, 16) == E.NULL_POINTER
    assert A(0, f4, 16, f4, 16, f4, 16, 2, i4, 1, 1, 1, 16, None, 16) == E.NULL_POINTER
    G = L.kjarni_hip_op_score_gather_norm
    assert G(0, None, 16, 1, i4, 1, 16, f4, None, 1e-6, lp, 16) == E.NULL_POINTER
    assert G(0, f4, 16, 1, None, 1, 16, f4, None, 1e-6, lp, 16) == E.NULL_POINTER
    assert G(0, f4, 16, 1, i4, 1, 16, None, None, 1e-6, lp, 16) == E.NULL_POINTER
    assert G(0, f4, 16, 1, i4, 1, 16, f4, None, 1e-6, None, 16) == E.NULL_POINTER
    res = (_ffi.KjarniScoreResult * 2)()
    res[0].n_tokens = 7
    ctx = (C.c_char_p * 2)(b"a", b"b")
    assert L.kjarni_generator_score_batch(None, ctx, ctx, 2, res) == E.NULL_POINTER
    assert L.kjarni_generator_score_batch(None, None, None, 0, None) == E.NULL_POINTER
    assert list(lp) == [9.0] * 4 and list(top) == [9] * 4 and res[0].n_tokens == 7                                # nothing written


# ---- the plan -------------------------------------------------------------------------------------------------------------------

def _lcp(a, b):
    k = 0
    while k < min(len(a), len(b)) and a[k] == b[k]:
        k += 1
    return k


def _plan(seqs, firsts, head_dim, min_shared):
    """The rule of the issue, restated: chunks (first sequence, rows), groups, the three block tables and the gather table."""
    B = len(seqs)
    lens = [len(s) for s in seqs]
    slot0 = np.concatenate([[0], np.cumsum([n - f for n, f in zip(lens, firsts)])]).tolist()
    units, i = [], 0
    while i < B:
        p, j = firsts[i], i + 1
        while j < B:
            q = min(p, firsts[j], _lcp(seqs[i], seqs[j]))
            if q < min_shared:
                break
            if q + sum(lens[t] - q for t in range(i, j + 1)) > 2048:
                break
            if max(lens[t] - q for t in range(i, j + 1)) >= 256:
                break
            p, j = q, j + 1
        if j - i >= 2:
            units.append((i, j, p))
        else:
            j = i + 1
            units.append((i, j, 0))
        i = j
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
            for pos in range(firsts[t], lens[t]):
                src = row + (pos - 1 - p) if pos - 1 >= p else pf + p - 1
                gather.append((c, src, seqs[t][pos], slot0[t] + pos - firsts[t]))
            row += own
        chunks[-1][1] = row
    return {"chunk_first_seq": [c[0] for c in chunks] + [B], "chunk_rows": [c[1] for c in chunks], "groups": groups, "vec": vec, "mfma": mfma,
            "prefix": pre, "gather": gather}


def _seqs(spec, seed=3, vocab=1000):
    """spec: (context key, context length, continuation length) per sequence; equal keys share the context's tokens, and every
    continuation starts with a token of its own, so that the common prefix of two sharers is exactly the context."""
    rng = np.random.default_rng(seed)
    ctx, out, firsts = {}, [], []
    for n, (key, clen, tail) in enumerate(spec):
        if key not in ctx:
            ctx[key] = [vocab + 10 * len(ctx)] + rng.integers(0, vocab, clen - 1).tolist()     # (a first token no other context has)
        out.append(ctx[key][:clen] + [2000 + n] + rng.integers(0, vocab, tail - 1).tolist())
        firsts.append(clen)
    return out, firsts


CASES = {
    "no_common_prefix": (_seqs([("a", 5, 3), ("b", 7, 2), ("c", 3, 9)]), 64, 1),
    "four_way_group": (_seqs([("a", 12, 1), ("a", 12, 3), ("a", 12, 8), ("a", 12, 17)]), 64, 1),
    "two_groups_and_a_plain": (_seqs([("a", 40, 2), ("a", 40, 5), ("b", 9, 4), ("c", 33, 1), ("c", 33, 70), ("c", 33, 3)]), 32, 1),
    "below_min_shared": (_seqs([("a", 3, 4), ("a", 3, 6), ("b", 8, 2), ("b", 8, 2)]), 64, 4),
    "cut_by_2048_rows": (_seqs([("a", 100, 250)] * 9), 64, 1),                   # 100 + 8 * 250 > 2048: the ninth starts a new unit
    "remainder_of_256_ends_the_group": (_seqs([("a", 20, 10), ("a", 20, 255), ("a", 20, 256), ("a", 20, 5)]), 64, 1),
    "group_closes_the_chunk": (_seqs([("x", 900, 100), ("y", 900, 100), ("a", 30, 10), ("a", 30, 10), ("a", 30, 10)]), 64, 1),
    "interleaved_sharers": (_seqs([("a", 10, 2), ("b", 10, 2), ("a", 10, 3), ("b", 10, 3)]), 64, 1),
    "mfma_prefix": (_seqs([("a", 300, 5), ("a", 300, 40), ("a", 300, 12)]), 64, 1),
    "long_prefix_on_the_vector_route": (_seqs([("a", 300, 5), ("a", 300, 40)]), 32, 1),
}


def _capped_by_the_smallest_first():
    """Three sequences with 20 common tokens whose firsts are 20, 6 and 20: the group's prefix is 6."""
    seqs, firsts = _seqs([("a", 20, 4), ("a", 20, 9), ("a", 20, 2)])
    firsts[1] = 6
    return (seqs, firsts), 64, 1


CASES["capped_by_the_smallest_first"] = _capped_by_the_smallest_first()


@pytest.mark.parametrize("name", sorted(CASES))
def test_score_plan_matches_the_rule(name):
    (seqs, firsts), head_dim, min_shared = CASES[name]
    got = kjarni_amd.score_plan(seqs, firsts, head_dim, min_shared)
    want = _plan(seqs, firsts, head_dim, min_shared)
    for key in want:
        assert [tuple(r) if isinstance(r, list) else r for r in got[key].tolist()] == want[key], key
    lens = [len(s) for s in seqs]
    # what each case is about
    groups = [tuple(g) for g in got["groups"].tolist()]
    if name == "no_common_prefix":
        assert groups == [] and len(got["prefix"]) == 0 and sum(got["chunk_rows"]) == sum(lens)
    if name == "four_way_group":
        assert groups == [(0, 0, 4, 12)] and got["chunk_rows"].tolist() == [12 + 1 + 3 + 8 + 17]
    if name == "capped_by_the_smallest_first":
        assert groups == [(0, 0, 3, 6)]
    if name == "below_min_shared":
        assert groups == [(0, 2, 2, 8)]
    if name == "cut_by_2048_rows":
        assert groups == [(0, 0, 7, 100), (1, 7, 2, 100)] and got["chunk_rows"].tolist() == [100 + 7 * 250, 100 + 2 * 250]
    if name == "remainder_of_256_ends_the_group":
        assert groups == [(0, 0, 2, 20)]                      # the 256-row remainder ends the group, and can lead none itself
    if name == "group_closes_the_chunk":
        assert groups == [(1, 2, 3, 30)] and got["chunk_first_seq"].tolist() == [0, 2, 5] and got["chunk_rows"].tolist() == [2000, 60]
    if name == "interleaved_sharers":
        assert groups == []
    if name == "mfma_prefix":
        assert [tuple(b) for b in got["mfma"].tolist()] == [(0, 0, 0, 300), (0, 0, 128, 300), (0, 0, 256, 300)] and len(got["vec"]) == 0
        assert [tuple(b) for b in got["prefix"].tolist()] == [(0, 300, 0, 5, 0, 300), (0, 305, 0, 40, 0, 300), (0, 305, 32, 40, 0, 300),
                                                              (0, 345, 0, 12, 0, 300)]
    if name == "long_prefix_on_the_vector_route":
        assert len(got["mfma"]) == 0 and len(got["vec"]) == 10
    # invariants: every scored position has one gather entry, its slots are 0 .. S - 1 in order, its rows lie inside its chunk
    S = sum(n - f for n, f in zip(lens, firsts))
    assert got["gather"][:, 3].tolist() == list(range(S))
    for c, src, tgt, slot in got["gather"].tolist():
        assert 0 <= src < got["chunk_rows"][c]
    assert (got["chunk_rows"] <= 2048).all()
    saved = sum((m - 1) * p for _, _, m, p in groups)
    assert sum(got["chunk_rows"]) == sum(lens) - saved


def test_score_plan_on_random_batches():
    rng = np.random.default_rng(5)
    for trial in range(20):
        spec = []
        for _ in range(int(rng.integers(1, 40))):
            key, clen = int(rng.integers(0, 6)), int(rng.integers(1, 60))
            spec += [(key * 100 + clen, clen, int(rng.integers(1, 300))) for _ in range(int(rng.integers(1, 5)))]
        seqs, firsts = _seqs(spec, seed=trial)
        firsts = [int(rng.integers(1, f + 1)) if rng.random() < 0.2 else f for f in firsts]
        for head_dim, min_shared in ((64, 1), (32, 8)):
            got = kjarni_amd.score_plan(seqs, firsts, head_dim, min_shared)
            want = _plan(seqs, firsts, head_dim, min_shared)
            for key in want:
                assert [tuple(r) if isinstance(r, list) else r for r in got[key].tolist()] == want[key], (trial, key)


def test_gather_table_by_hand():
    """Two contexts; A = [1, 2, 3] is followed by [4], [5, 6] and (scored from position 2, inside the context) [7]; B = [8, 9] by
    [10, 11] alone.  The group's prefix is capped at 2 by the third member's first, so members 0 and 1 -- whose first is 3 --
    read their first scored position's source row in their own remainder, and member 2 reads the prefix's last row."""
    seqs = [[1, 2, 3, 4], [1, 2, 3, 5, 6], [1, 2, 3, 7], [8, 9, 10, 11]]
    firsts = [3, 3, 2, 2]
    got = kjarni_amd.score_plan(seqs, firsts, 64, 1)
    assert got["groups"].tolist() == [[0, 0, 3, 2]]
    # rows: 0-1 prefix [1, 2]; 2-3 [3, 4]; 4-6 [3, 5, 6]; 7-8 [3, 7]; 9-12 the plain sequence
    assert got["chunk_rows"].tolist() == [13]
    assert got["prefix"].tolist() == [[0, 2, 0, 2, 0, 2], [0, 4, 0, 3, 0, 2], [0, 7, 0, 2, 0, 2]]
    assert got["vec"].tolist() == [[0, 0, 0, 2], [0, 9, 0, 4]]
    assert got["gather"].tolist() == [[0, 2, 4, 0],                      # seq 0, pos 3: position 2 is row 2
                                      [0, 4, 5, 1], [0, 5, 6, 2],        # seq 1, pos 3 and 4
                                      [0, 1, 3, 3], [0, 7, 7, 4],        # seq 2, pos 2: the prefix's last row; pos 3: its own row 7
                                      [0, 10, 10, 5], [0, 11, 11, 6]]    # the plain sequence, pos 2 and 3
    # every member whose first equals the prefix length lists the prefix's last row once
    seqs = [[1, 2, 3], [1, 2, 4, 5], [1, 2, 6]]
    got = kjarni_amd.score_plan(seqs, [2, 2, 2], 64, 1)
    assert got["groups"].tolist() == [[0, 0, 3, 2]]
    assert got["gather"].tolist() == [[0, 1, 3, 0], [0, 1, 4, 1], [0, 3, 5, 2], [0, 1, 6, 3]]


def test_score_plan_refusals():
    for seqs, firsts, words in (([[1]], [1], "fewer than 2"), ([[1, 2], [3, 4]], [1, 2], "firsts[1]"), ([[1, 2]], [0], "firsts[0]"),
                                ([[1, 2], list(range(2049))], [1, 1], "(sequence 1)")):
        with pytest.raises(KjarniException) as e:
            kjarni_amd.score_plan(seqs, firsts)
        assert e.value.code == E.INVALID_CONFIG and words in str(e.value), str(e.value)
    with pytest.raises(KjarniException) as e:
        kjarni_amd.score_plan([[1, 2]], [1], min_shared=0)
    assert e.value.code == E.INVALID_CONFIG and "min_shared" in str(e.value)
    ids, off, fs = (C.c_uint32 * 4)(1, 2, 3, 4), (C.c_int32 * 3)(0, 3, 1), (C.c_int32 * 2)(1, 1)
    n = [C.c_int32() for _ in range(6)]
    rc = L.kjarni_hip_score_plan(ids, off, fs, 2, 64, 1, None, None, C.byref(n[0]), None, 0, C.byref(n[1]), None, 0, C.byref(n[2]), None, 0,
                                 C.byref(n[3]), None, 0, C.byref(n[4]), None, 0, C.byref(n[5]))
    assert rc == E.INVALID_CONFIG and "offsets must not decrease" in _ffi.last_error()
    empty = kjarni_amd.score_plan([], [])
    assert empty["chunk_first_seq"].tolist() == [0] and all(len(empty[k]) == 0 for k in ("groups", "vec", "mfma", "prefix", "gather"))
