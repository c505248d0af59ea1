"""Decoder rerankers on the GPU (kjarni_hip_op_answer_logits, kjarni_hip_decoder_answer_logits, kjarni_reranker_* on a decoder
checkpoint).

The kernel alone against numpy float64, with everything it must not read set to NaN; whole models -- independent sequences, one
query in front of several documents, two queries interleaved -- against the float64 references run sequence by sequence and
against forward(); chunks; the state a call leaves; refusals; the Reranker end to end.

Bars.  Logits: the flat 1e-4 of the README's parity section against float64 (the inputs are scaled as the fixtures scale them, so
the float64 logits stay O(1)), 2e-4 where two device results are compared (both carry the bar).  Scores: the sigmoid's slope is
at most 1/4, so the logit bar carries over.  Every figure is printed before it is asserted."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from tests import gguf_fixture as GG
from tests import qwen3_fixture as F
from tests import rerank_fixture as RF
from tests import synth
from tests.test_gpu_score import _bf16_round, _w_arg
from tests.test_gpu_score_batch import _Case

pytestmark = pytest.mark.gpu
F64 = np.float64
BAR = 1e-4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _within(got, ref, what, bar=BAR):
    ref = np.asarray(ref, F64)
    assert np.shape(got) == ref.shape, what
    err = float(np.abs(np.asarray(got, F64) - ref).max())
    print(f"{what}: err {err:.3e} bar {bar:.1e} max |ref| {float(np.abs(ref).max()):.2f}")
    assert np.isfinite(got).all() and err <= bar, f"{what}: {err:.3e} > {bar:.1e}"


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------

TARGET_SETS = {1: [6], 2: [9, 2], 8: [3, 7, 3, 0, 10, 5, 1, 8]}        # (8: a target listed twice)
SRC = [4, 1, 4, 6]                                                     # (a row listed twice)


def _kernel_case(hidden, bf16, form):
    """x [8, ldx] and head [11, hidden] (0.1 N(0, 1), as the fixtures draw the embedding), gamma, beta.  ldx = hidden + 4 at 64 and
    1 024 (16-byte rows: the LayerNorm form takes launch_layernorm's float4 arithmetic), hidden + 5 elsewhere (rows at any
    4-byte alignment); the head rows of 33 elements start at every alignment their type allows."""
    rng = np.random.default_rng(hidden * 4 + 2 * int(bf16) + (form == "layernorm"))
    x = rng.standard_normal((8, hidden + (4 if hidden % 8 == 0 else 5))).astype(np.float32)
    head = (rng.standard_normal((11, hidden), dtype=np.float32) * np.float32(0.1))
    if bf16:
        head = _bf16_round(head)
    gamma = (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(hidden)).astype(np.float32) if form == "layernorm" else None
    return x, head, gamma, beta


def _kernel_ref(x, head, gamma, beta, eps, hidden, src, targets):
    rows = x[src, :hidden].astype(F64)
    if beta is None:
        n = rows / np.sqrt((rows * rows).mean(-1, keepdims=True) + eps) * gamma.astype(F64)
    else:
        mean = rows.mean(-1, keepdims=True)
        n = (rows - mean) / np.sqrt(((rows - mean) ** 2).mean(-1, keepdims=True) + eps) * gamma.astype(F64) + beta.astype(F64)
    return n @ head[targets].astype(F64).T


@pytest.mark.parametrize("form", ["rms", "layernorm"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("hidden", [4, 33, 64, 1024, 4100])
def test_kernel_against_float64_and_reads_nothing_else(hidden, bf16, form):
    from kjarni_amd import ops
    x, head, gamma, beta = _kernel_case(hidden, bf16, form)
    eps = 1e-6 if form == "rms" else 1e-5
    for k, targets in TARGET_SETS.items():
        want = _kernel_ref(x, head, gamma, beta, eps, hidden, SRC, targets)
        got = ops.answer_logits(x, SRC, gamma, _w_arg(head, bf16), targets, beta, eps, hidden, head_is_bf16=bf16)
        assert got.shape == (len(SRC), k)
        _within(got, want, f"hidden {hidden} bf16 {bf16} {form} targets {k}")
        assert np.array_equal(_bits(got[0]), _bits(got[2]))                                     # the row listed twice
        if k == 8:
            assert np.array_equal(_bits(got[:, 0]), _bits(got[:, 2]))                             # the target listed twice
        # everything the kernel must not read is NaN: the other rows of x, the padding behind hidden, the head rows not targeted
        xn, hn = np.full_like(x, np.nan), np.full_like(head, np.nan)
        xn[SRC, :hidden] = x[SRC, :hidden]
        hn[targets] = head[targets]
        again = ops.answer_logits(xn, SRC, gamma, _w_arg(hn, bf16), targets, beta, eps, hidden, head_is_bf16=bf16)
        assert np.isfinite(again).all(), f"hidden {hidden} targets {k}: NaN leaked in"
        assert np.array_equal(_bits(again), _bits(got)), f"hidden {hidden} targets {k}: the result changed with what it must not read"


def test_kernel_hook_validates():
    from kjarni_amd import ops
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    x, head, g = np.zeros((5, 36), np.float32), np.zeros((7, 32), np.float32), np.ones(32, np.float32)
    assert ops.answer_logits(x, [0, 4], g, head, [0, 6], hidden=32).shape == (2, 2)
    for kw, words in ((dict(src=[0, 5]), "src[1]"), (dict(src=[-1]), "src[0]"), (dict(targets=[0, 7]), "targets[1]"),
                      (dict(targets=list(range(7)) + [0, 1]), "n_targets"), (dict(targets=[]), "n_targets")):
        args = dict(src=[0, 4], targets=[0, 6]) | kw
        with pytest.raises(KjarniException) as e:
            ops.answer_logits(x, args["src"], g, head, args["targets"], hidden=32)
        assert e.value.code == E.INVALID_CONFIG and words in str(e.value), str(e.value)
    with pytest.raises(KjarniException) as e:
        ops.answer_logits(np.zeros((5, 30), np.float32), [0], g, head, [0], hidden=32)            # ldx below hidden
    assert e.value.code == E.INVALID_CONFIG and "ldx" in str(e.value)


# ---- 2. whole models ---------------------------------------------------------------------------------------------------------------

MISTRAL = dict(model_type="mistral", rope_theta=10000.0, tie_word_embeddings=False)
MODELS = [(name, kind, over, bf16) for name, kind, over in (("llama", "llama", {}), ("qwen2", "qwen2", {}), ("mistral", "llama", MISTRAL),
                                                           ("Q3_SMALL", "Q3_SMALL", {}), ("Q3_EVEN", "Q3_EVEN", {}), ("Q3_D128", "Q3_D128", {}),
                                                           ("gpt2", "gpt2", {})) for bf16 in (False, True)]
MODEL_IDS = [f"{m[0]}{'-bf16' if m[3] else ''}" for m in MODELS]
INDEPENDENT = [2, 5, 30, 9, 64, 24]
QUERY_LEN, DOCUMENT_LENS = 20, [3, 40, 7, 12, 25, 33]


def _batches(case):
    rng = np.random.default_rng(31)
    draw = lambda n: rng.integers(case.first_id, case.vocab, n).tolist()  # noqa: E731
    independent = [draw(n) for n in INDEPENDENT]
    qa, qb = draw(QUERY_LEN), draw(QUERY_LEN)
    qb[0] = qa[0] + 1 if qa[0] + 1 < case.vocab else qa[0] - 1                                   # (the two queries differ from their first token on)
    shared = [qa + draw(n) for n in DOCUMENT_LENS]
    other = [qb + draw(n) for n in DOCUMENT_LENS[:3]]
    interleaved = [s for pair in zip(shared[:3], other) for s in pair]
    targets = rng.choice(np.arange(case.first_id, case.vocab), 7, replace=False).tolist()
    return independent, shared, interleaved, targets + targets[2:3]                              # (eight targets, one listed twice)


def _planned(dec, seqs):
    import kjarni_amd
    plan = kjarni_amd.answer_plan(seqs, dec.head_dim)
    return plan, (int(plan["chunk_rows"].sum()), int(sum((m - 1) * p for _, _, m, p in plan["groups"].tolist())))


def _forward(dec, ids):
    """The logits row forward() gives for `ids` run alone, from an empty cache."""
    dec.reset()
    return dec.forward(ids)[1]


def _check_batch(case, seqs, targets, what):
    """answer_logits(seqs, targets) against float64 sequence by sequence (1e-4); the counters against the plan."""
    dec = case.dec
    plan, (rows, saved) = _planned(dec, seqs)
    r0 = dec.answer_rows()
    got = dec.answer_logits(seqs, targets)
    r1 = dec.answer_rows()
    assert (r1[0] - r0[0], r1[1] - r0[1]) == (rows, saved), what
    assert got.shape == (len(seqs), len(targets))
    want = np.stack([case.logits(s)[len(s) - 1, targets] for s in seqs])
    _within(got, want, what)
    return got, plan, saved


@pytest.mark.parametrize("name,kind,over,bf16", MODELS, ids=MODEL_IDS)
def test_models_against_float64_and_forward(tmp_path, name, kind, over, bf16):
    case = _Case(tmp_path, kind, bf16, **over)
    dec = case.dec
    assert dec.config.get("model_type", "gpt2") == ("qwen3" if name.startswith("Q3") else name)
    independent, shared, interleaved, targets = _batches(case)
    score_rows = dec.score_batch_rows()
    got, plan, saved = _check_batch(case, independent, targets, f"{name} independent")
    assert len(plan["groups"]) == 0 and saved == 0
    for i, s in enumerate(independent):
        _within(got[i], _forward(dec, s)[targets], f"{name} independent sequence {i} against forward()", 2 * BAR)
    got, plan, saved = _check_batch(case, shared, targets, f"{name} one query, six documents")
    assert [tuple(g) for g in plan["groups"].tolist()] == [(0, 0, 6, QUERY_LEN)] and saved == 5 * QUERY_LEN > 0
    for i, s in enumerate(shared):
        _within(got[i], _forward(dec, s)[targets], f"{name} shared sequence {i} against forward()", 2 * BAR)
    two = dec.answer_logits(shared, targets[:2])                                                  # the reranker's K = 2: the same arithmetic per target
    assert np.array_equal(_bits(two), _bits(got[:, :2]))
    mixed, plan, saved = _check_batch(case, interleaved, targets, f"{name} two queries interleaved")
    assert len(plan["groups"]) == 0 and saved == 0
    for i, s in enumerate(interleaved):
        _within(mixed[i], _forward(dec, s)[targets], f"{name} interleaved sequence {i} against forward()", 2 * BAR)
    for slot in range(0, 6, 2):                                                                   # and shared against not shared
        _within(mixed[slot], got[slot // 2], f"{name} sequence {slot // 2}: not shared against shared", 2 * BAR)
    one = dec.answer_logits(interleaved, targets[:1])                                             # K = 1
    assert np.array_equal(_bits(one), _bits(mixed[:, :1]))
    assert dec.score_batch_rows() == score_rows                                                   # score_batch's counters are its own


# ---- 3. chunks ---------------------------------------------------------------------------------------------------------------------

def test_more_than_one_chunk_and_a_group_split_by_the_chunk(tmp_path):
    case = _Case(tmp_path, "llama", False, max_position_embeddings=512)
    rng = np.random.default_rng(41)
    draw = lambda n: rng.integers(case.first_id, case.vocab, n).tolist()  # noqa: E731
    seqs = [draw(120) for _ in range(20)]
    got, plan, saved = _check_batch(case, seqs, [7, 11], "20 x 120 tokens")
    assert plan["chunk_first_seq"].tolist() == [0, 17, 20] and plan["chunk_rows"].tolist() == [17 * 120, 3 * 120] and saved == 0
    # a query of 100 tokens in front of nine documents of 250: 100 + 9 x 250 rows do not fit one chunk, so the group is split
    query = draw(100)
    seqs = [query + draw(250) for _ in range(9)]
    got, plan, saved = _check_batch(case, seqs, [7, 11], "9 x (100 + 250) tokens")
    assert [tuple(g) for g in plan["groups"].tolist()] == [(0, 0, 7, 100), (1, 7, 2, 100)] and saved == 7 * 100
    assert plan["chunk_rows"].tolist() == [100 + 7 * 250, 100 + 2 * 250]


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------

def test_leaves_generation_and_scoring_state_untouched(tmp_path):
    case = _Case(tmp_path, "llama", False)
    dec = case.dec
    independent, shared, interleaved, targets = _batches(case)
    firsts = [QUERY_LEN] * len(shared)
    rng = np.random.default_rng(9)
    prompt = rng.integers(4, case.vocab, 30).tolist()
    first = dec.generate(prompt, 8)
    scored = dec.score(prompt, 5)
    batch = dec.score_batch(shared, firsts, 2)
    state = (dec.cache_len(), dec.resident(), _bits(dec.last_logits()).copy(), dec.prefix_stats(), dec.score_batch_rows(), dec.score_calls())
    kv = [tuple(a.copy() for a in dec.kv_rows(i)) for i in range(dec.layers)]
    dec.answer_logits(shared + independent, targets)
    assert (dec.cache_len(), dec.resident()) == state[:2] and np.array_equal(_bits(dec.last_logits()), state[2])
    assert (dec.prefix_stats(), dec.score_batch_rows(), dec.score_calls()) == state[3:]
    for i in range(dec.layers):
        k, v = dec.kv_rows(i)
        assert np.array_equal(_bits(k), _bits(kv[i][0])) and np.array_equal(_bits(v), _bits(kv[i][1]))
    same = lambda a, b: np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b)  # noqa: E731
    assert all(same(a, b) for a, b in zip(batch, dec.score_batch(shared, firsts, 2)))
    assert dec.generate(prompt, 8) == first
    assert all(same(a, b) for a, b in zip(scored, dec.score(prompt, 5)))
    a0 = dec.answer_rows()
    dec.generate(prompt, 4), dec.score(prompt, 5), dec.score_batch(shared, firsts)
    assert dec.answer_rows() == a0                                                                # and the new counters are their own


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------

def test_validates_before_any_gpu_work(tmp_path):
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    case = _Case(tmp_path, "qwen2", False)                    # max_position_embeddings 128: the length limit
    dec, V = case.dec, case.vocab
    ids = np.arange(4, 4 + 200, dtype=np.uint32) % (V - 4) + 4
    dec.forward([5, 6, 7], fetch=False)
    cases = [
        (ids, [0, 5, 3, 9], [5, 6], ("offsets[2]", "sequence 1")),            # offsets that decrease
        (ids, [0, 5, 6, 9], [5, 6], ("fewer than 2", "sequence 1")),          # a sequence of one token
        (ids, [0, 5, 5, 9], [5, 6], ("fewer than 2", "sequence 1")),          # an empty one
        (ids, [0, 5, 134], [5, 6], ("offsets", "129", "128", "sequence 1")),  # longer than min(context, 2048)
        (ids, [-1, 3], [5, 6], ("offsets[0]",)),
        (ids, [0, 5, 9], [], ("n_targets", "0")),
        (ids, [0, 5, 9], list(range(4, 13)), ("n_targets", "9")),
        (ids, [0, 5, 9], [5, V], ("targets[1]", str(V))),
    ]
    bad = ids.copy()
    bad[7] = V
    cases.append((bad, [0, 5, 9], [5, 6], ("ids[7]", str(V), "sequence 1")))
    before = (dec.answer_rows(), dec.tile_gemm_calls())
    for a, off, targets, words in cases:
        with pytest.raises(KjarniException) as e:
            dec.answer_logits_flat(a, off, targets)
        assert e.value.code == E.INVALID_CONFIG and all(w in str(e.value) for w in words), str(e.value)
    assert dec.cache_len() == 3 and (dec.answer_rows(), dec.tile_gemm_calls()) == before
    assert dec.answer_logits([], [5, 6]).shape == (0, 2) and dec.answer_rows() == before[0]      # B == 0 writes nothing
    assert dec.answer_logits_flat(ids, [0, 128], [5]).shape == (1, 1)                             # exactly the limit is fine


def test_refuses_quantized_and_odd_geometries(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    path = str(tmp_path / "q8.gguf")
    GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    dec = kjarni_amd.HipDecoder(path)
    with pytest.raises(KjarniException) as e:
        dec.answer_logits([[5, 6, 7]], [5, 6])
    assert e.value.code == E.INVALID_CONFIG and "quantized" in str(e.value) and dec.answer_rows() == (0, 0)
    d = str(tmp_path / "odd")      # hidden 48: not a multiple of 32, the packed path's own rule
    synth.llm_model(d, dict(synth.LLAMA_TEST, hidden_size=48, num_attention_heads=3, num_key_value_heads=1, head_dim=16, intermediate_size=96), seed=3)
    dec = kjarni_amd.HipDecoder(d)
    with pytest.raises(KjarniException) as e:
        dec.answer_logits([[5, 6, 7]], [5, 6])
    assert e.value.code == E.INVALID_CONFIG and "multiples of 32" in str(e.value) and dec.answer_rows() == (0, 0)


# ---- 6. the Reranker ---------------------------------------------------------------------------------------------------------------

def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, F64)))


def test_reranker_on_a_decoder_checkpoint(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    from kjarni_amd.reranker import rerank_prompt_ids
    from tests.qwen3_ref64 import Qwen3Ref64
    d = str(tmp_path / "reranker")
    cfg, t = F.qwen3_model(d, F.Q3_SMALL, seed=RF.MODEL_SEED, std=RF.MODEL_STD, vocab_size=RF.VOCAB, max_position_embeddings=RF.MAX_POSITIONS,
                           bos_token_id=700, eos_token_id=702)
    tok = RF.write_tokenizer(os.path.join(d, "tokenizer.json"))
    ref = Qwen3Ref64(t, cfg)

    def oracle(docs, instruction=None, limit=RF.MAX_POSITIONS):
        out = []
        for doc in docs:
            ids = rerank_prompt_ids(tok, RF.QUERY, doc, instruction, limit)
            lg = ref.logits(ref.forward(list(ids), ref.new_cache())[-1:])[0]
            out.append(float(_sigmoid(lg[RF.YES] - lg[RF.NO])))
        return np.array(out, F64)
    want = oracle(RF.DOCUMENTS)
    gap = float(np.diff(np.sort(want)).min())
    print(f"float64 scores {np.round(want, 4).tolist()}; the closest two are {gap:.3e} apart")
    assert gap > 100 * BAR, f"precondition: two float64 scores lie within {gap:.2e}"
    rr = kjarni_amd.Reranker(model_path=d)
    assert rr.answer_rows() == (0, 0)
    res = rr.rerank(RF.QUERY, RF.DOCUMENTS)
    rows, saved = rr.answer_rows()
    got = np.zeros(len(RF.DOCUMENTS))
    for r in res:
        got[r.index] = r.score
    _within(got, want, "rerank scores against float64")
    order = sorted(range(len(want)), key=lambda i: -want[i])
    assert [r.index for r in res] == order and [r.document for r in res] == [RF.DOCUMENTS[i] for i in order]
    # the system block, the instruction and the query were computed once
    lens = [len(rerank_prompt_ids(tok, RF.QUERY, doc)) for doc in RF.DOCUMENTS]
    assert saved >= 7 * len(kjarni_amd.BpeTokenizer(tok).encode(RF.HEAD)) > 0 and rows == sum(lens) - saved
    top = rr.rerank_top_k(RF.QUERY, RF.DOCUMENTS, 3)
    assert [(r.index, r.score) for r in top] == [(r.index, r.score) for r in res[:3]]
    assert rr.rerank(RF.QUERY, []) == []
    for i in (0, 5):
        one = rr.score(RF.QUERY, RF.DOCUMENTS[i])
        _within(np.array([one]), want[i:i + 1], f"score() of document {i} against float64")
        # score() is rerank() of that one document: the same call, the same bits.  Inside the batch of eight the document's rows
        # attend to the shared prefix through the prefix attention kernel, alone they take the plain route: two device results
        # of different arithmetic, each within the bar of float64, hence 2 x the bar between them.
        assert rr.rerank(RF.QUERY, [RF.DOCUMENTS[i]])[0].score == one
        assert abs(one - got[i]) <= 2 * BAR
    # the instruction changes the ids and the scores; None restores both
    assert rerank_prompt_ids(tok, RF.QUERY, RF.DOCUMENTS[0], RF.OTHER_INSTRUCTION) != rerank_prompt_ids(tok, RF.QUERY, RF.DOCUMENTS[0])
    other = oracle(RF.DOCUMENTS, RF.OTHER_INSTRUCTION)
    assert float(np.abs(other - want).max()) > 100 * BAR
    rr.set_instruction(RF.OTHER_INSTRUCTION)
    changed = np.zeros(len(RF.DOCUMENTS))
    for r in rr.rerank(RF.QUERY, RF.DOCUMENTS):
        changed[r.index] = r.score
    _within(changed, other, "rerank scores under another instruction against float64")
    rr.set_instruction(None)
    back = rr.rerank(RF.QUERY, RF.DOCUMENTS)
    assert [(r.index, r.score) for r in back] == [(r.index, r.score) for r in res]
    with pytest.raises(KjarniException) as e:
        kjarni_amd._ffi.check_error(kjarni_amd.lib().kjarni_reranker_set_instruction(rr._handle, b"\xff\xfe"))
    assert e.value.code == E.INVALID_UTF8
    # a long document is cut, not refused: its score is the float64 score of the cut prompt
    long_doc = "The Seine runs through Paris. " * 80
    assert len(kjarni_amd.BpeTokenizer(tok).encode(long_doc)) > RF.MAX_POSITIONS
    cut = rerank_prompt_ids(tok, RF.QUERY, long_doc, None, RF.MAX_POSITIONS)
    assert len(cut) == RF.MAX_POSITIONS
    _within(np.array([rr.score(RF.QUERY, long_doc)]), oracle([long_doc]), "a document cut to the length limit")
    with pytest.raises(KjarniException) as e:                                                       # a query that does not fit is refused
        rr.score("Which river? " * 200, "The Seine.")
    assert e.value.code == E.INVALID_CONFIG and "reach into the query" in str(e.value)


def test_reranker_loads_by_name_and_refuses_a_tokenizer_without_yes(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    cache = tmp_path / "cache"
    d = str(cache / "Qwen_Qwen3-Reranker-0.6B")
    F.qwen3_model(d, F.Q3_SMALL, seed=RF.MODEL_SEED, std=RF.MODEL_STD, vocab_size=RF.VOCAB, max_position_embeddings=RF.MAX_POSITIONS)
    RF.write_tokenizer(os.path.join(d, "tokenizer.json"))
    by_name = kjarni_amd.Reranker("Qwen/Qwen3-Reranker-0.6B", cache_dir=str(cache))
    by_path = kjarni_amd.Reranker(model_path=d)
    assert by_name.score(RF.QUERY, RF.DOCUMENTS[0]) == by_path.score(RF.QUERY, RF.DOCUMENTS[0])
    shutil.copy(os.path.join(RF.GOLDEN, "bpe_qwen2_tokenizer.json"), os.path.join(d, "tokenizer.json"))
    with pytest.raises(KjarniException) as e:
        kjarni_amd.Reranker(model_path=d)
    assert e.value.code == E.LOAD_FAILED and '"yes"' in str(e.value)


def test_set_instruction_on_a_cross_encoder_is_refused_and_changes_nothing(tmp_path):
    import kjarni_amd
    from kjarni_amd._ffi import KjarniError as E
    from kjarni_amd._ffi import KjarniException
    d = str(tmp_path / "ce")
    synth.minilm_cross_encoder(d, seed=4)
    synth.add_tokenizer(d)
    rr = kjarni_amd.Reranker(model_path=d)
    docs = ["Reykjavik is the capital of Iceland.", "Whales are mammals.", "The capital of France is Paris."]
    before = [(r.index, r.score) for r in rr.rerank("what is the capital of iceland", docs)]
    with pytest.raises(KjarniException) as e:
        rr.set_instruction("Find the capital")
    assert e.value.code == E.INVALID_CONFIG and "cross-encoder" in str(e.value)
    with pytest.raises(KjarniException) as e:
        rr.set_instruction(None)
    assert e.value.code == E.INVALID_CONFIG
    assert [(r.index, r.score) for r in rr.rerank("what is the capital of iceland", docs)] == before and rr.answer_rows() == (0, 0)
