"""Constrained decoding, host side (no GPU): the new symbols, their arities and what they do with NULL; the pattern compiler
against Python's re (full match and liveness over enumerated strings, the flags by graph search, every refusal with its
message); BpeTokenizer.token_bytes on tokenizers the test writes; the pattern builders of kjarni_amd.constraints."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd import constraints as K
from kjarni_amd._ffi import KjarniError as E
from tests import constraint_cases as CC

SYMBOLS = {
    "kjarni_hip_regex_compile": 2, "kjarni_hip_regex_free": 1, "kjarni_hip_regex_dims": 3, "kjarni_hip_regex_table": 4,
    "kjarni_hip_regex_step": 5, "kjarni_bpe_tokenizer_token_bytes": 5, "kjarni_hip_constraint_new": 6, "kjarni_hip_constraint_free": 1,
    "kjarni_hip_constraint_dims": 4, "kjarni_hip_constraint_mask": 3, "kjarni_hip_constraint_counts": 2,
    "kjarni_hip_op_constraint_mask": 8, "kjarni_hip_op_constraint_apply": 10, "kjarni_hip_op_constraint_advance": 9,
    "kjarni_hip_decoder_generate_constrained": 11, "kjarni_hip_generator_set_constraint": 2, "kjarni_hip_chat_set_constraint": 2,
    "kjarni_hip_generator_constraint_result": 2, "kjarni_hip_chat_constraint_result": 2,
}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kjarni_hip.h")


# ---- 1. symbols and NULL behaviour -------------------------------------------------------------------------------------------------

def test_symbols_and_arities():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    assert callable(kjarni_amd.HipDecoder.generate_constrained)
    assert callable(kjarni_amd.Generator.set_constraint) and callable(kjarni_amd.Chat.set_constraint)
    assert callable(kjarni_amd.BpeTokenizer.token_bytes)
    for name in ("choices", "integer", "number", "json_string", "json_object"):
        assert callable(getattr(K, name))


def test_the_header_declares_what_ffi_mirrors():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, argc in SYMBOLS.items():
        m = re.search(r"\b(\w[\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in kjarni_hip.h"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == argc, name
        assert (_ffi.SIGNATURES[name][0] is C.c_int32) == ("KjarniErrorCode" in m.group(1)), name
    assert re.search(r"#define\s+KJARNI_CONSTRAINT_DEAD\s+0xFFFFu", text)
    assert re.search(r"#define\s+KJARNI_CONSTRAINT_MAX_STATES\s+4096", text)
    # the sampling options keep their layout: the constraint travels as an argument of its own
    assert "constraint" not in re.search(r"typedef struct KjarniHipSamplingOptions \{(.*?)\}", text, re.S).group(1)
    fields = [f for f, _ in _ffi.KjarniHipConstraintResult._fields_]
    assert fields == ["final_state", "device_state", "accepted", "complete", "violated"]
    m = re.search(r"typedef struct KjarniHipConstraintResult \{(.*?)\}", text, re.S)
    assert [w for w in re.findall(r"\w+", m.group(1)) if w in fields] == fields


def test_null_arguments():
    L = kjarni_amd.lib()
    h = C.c_void_p()
    assert L.kjarni_hip_regex_compile(None, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_regex_compile(b"a", None) == E.NULL_POINTER
    L.kjarni_hip_regex_free(None)
    L.kjarni_hip_constraint_free(None)
    n, s = C.c_int32(7), C.c_uint32(7)
    assert L.kjarni_hip_regex_dims(None, C.byref(n), C.byref(s)) == E.NULL_POINTER
    assert L.kjarni_hip_regex_table(None, None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_regex_step(None, 0, None, 0, C.byref(s)) == E.NULL_POINTER
    r = K.Regex("ab")
    assert L.kjarni_hip_regex_dims(r._h, None, None) == E.OK
    assert L.kjarni_hip_regex_table(r._h, None, None, None) == E.OK
    assert L.kjarni_hip_regex_step(r._h, 0, None, 0, None) == E.NULL_POINTER
    assert L.kjarni_hip_regex_step(r._h, 0, None, 2, C.byref(s)) == E.NULL_POINTER
    assert L.kjarni_hip_regex_step(r._h, 0, None, 0, C.byref(s)) == E.OK and s.value == r.start
    assert L.kjarni_hip_regex_step(r._h, 999, (C.c_uint8 * 1)(97), 1, C.byref(s)) == E.OK and s.value == CC.DEAD   # no such state
    nb = C.c_size_t(7)
    assert L.kjarni_bpe_tokenizer_token_bytes(None, 0, None, 0, C.byref(nb)) == E.NULL_POINTER
    off = np.zeros(3, np.uint32)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    assert L.kjarni_hip_constraint_new(0, None, u32(off), None, 2, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_constraint_new(0, r._h, None, None, 2, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_constraint_new(0, r._h, u32(off), None, 2, None) == E.NULL_POINTER
    # a malformed table is refused before any GPU work (so: here, without a GPU)
    bad = np.array([0, 2, 1], np.uint32)
    assert L.kjarni_hip_constraint_new(0, r._h, u32(bad), (C.c_uint8 * 2)(97, 98), 2, C.byref(h)) == E.INVALID_CONFIG
    assert "decreases" in _ffi.last_error()
    assert L.kjarni_hip_constraint_new(0, r._h, u32(np.array([0, 1, 2], np.uint32)), None, 2, C.byref(h)) == E.INVALID_CONFIG
    assert L.kjarni_hip_constraint_dims(None, None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_constraint_mask(None, 0, None) == E.NULL_POINTER
    assert L.kjarni_hip_constraint_counts(None, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_constraint_mask(0, None, 1, None, None, 1, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_constraint_apply(0, None, None, 1, 1, None, None, None, 0, None) == E.NULL_POINTER
    assert L.kjarni_hip_op_constraint_advance(0, None, None, 1, None, None, None, 0, None) == E.NULL_POINTER
    o = _ffi.KjarniHipSamplingOptions()
    o.max_new_tokens, o.repetition_penalty = 4, 1.0
    p, out, cnt = np.array([5, 6, 7], np.uint32), np.zeros(4, np.uint32), C.c_size_t(7)
    cb = _ffi.KjarniTokenCallbackFn()
    res = _ffi.KjarniHipConstraintResult(9, 9, 9, 9, 9)
    gen = L.kjarni_hip_decoder_generate_constrained
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(out), 4, C.byref(cnt), C.byref(res)) == E.NULL_POINTER
    assert cnt.value == 0 and (res.final_state, res.accepted, res.complete, res.violated) == (0, 0, 0, 0)
    assert gen(None, None, u32(p), 3, None, cb, None, u32(out), 4, C.byref(cnt), None) == E.NULL_POINTER
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(out), 4, None, None) == E.NULL_POINTER
    u = np.zeros(2, np.float32)
    o.uniforms, o.n_uniforms = u.ctypes.data_as(C.POINTER(C.c_float)), 2          # judged ahead of the handles
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(out), 4, C.byref(cnt), None) == E.INVALID_CONFIG
    assert L.kjarni_hip_generator_set_constraint(None, b"a") == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_constraint(None, None) == E.NULL_POINTER
    assert L.kjarni_hip_generator_constraint_result(None, C.byref(res)) == E.NULL_POINTER
    assert L.kjarni_hip_chat_constraint_result(None, None) == E.NULL_POINTER


# ---- 2, 3. the DFA against re: full match and liveness ---------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", list(CC.PATTERNS))
def test_full_match_and_liveness_against_re(pattern):
    r = K.Regex(pattern)
    alphabet, bound = CC.PATTERNS[pattern], CC.MAX_LEN[pattern]
    if bound == 0:   # the pattern of every escape matches exactly one string
        text = alphabet
        assert re.fullmatch(pattern, text, re.ASCII) and r.matches(text.encode())
        for cut in range(len(text)):
            q = r.step(r.start, text[:cut].encode())
            assert q != CC.DEAD and not r.accepting[q]
            assert r.step(r.start, (text[:cut] + "z").encode()) == CC.DEAD
        assert r.closed[r.step(r.start, text.encode())]
        return
    texts = list(CC.strings(alphabet, bound))
    matched = set()
    state = {}
    for t in texts:
        q = CC.walk(r.trans, r.start, t.encode())
        state[t] = q
        want = re.fullmatch(pattern, t, re.ASCII) is not None
        assert (q != CC.DEAD and bool(r.accepting[q])) == want, (pattern, t)
        if want:
            matched.add(t)
    assert matched, "precondition: the bound admits no match"
    # liveness: a prefix is alive iff some enumerated extension matches in full.  The check leaves nothing out when the shortest
    # completion from any live state fits the bound: asserted by a search over the table from every state a short string reaches.
    prefixes = set()
    for t in matched:
        for k in range(len(t) + 1):
            prefixes.add(t[:k])
    short = bound - _longest_completion(r)
    assert short >= 1, f"precondition: completions of {pattern!r} need up to {bound - short} characters"
    for t in texts:
        if len(t) <= short:
            assert (state[t] != CC.DEAD) == (t in prefixes), (pattern, t)


def _longest_completion(r) -> int:
    """The largest, over the states, of the fewest bytes to an accepting state (every byte is at most one character)."""
    S = r.states
    dist = np.where(r.accepting.astype(bool), 0, 10 ** 6)
    for _ in range(S):
        for q in range(S):
            nxt = [dist[t] for t in r.trans[q] if t != CC.DEAD]
            if nxt:
                dist[q] = min(dist[q], 1 + min(nxt))
    assert dist.max() < 10 ** 6, "a state of the table cannot reach an accepting state"
    return int(dist.max())


def test_non_ascii_is_matched_as_well_formed_utf8_only():
    r = K.Regex(r".")
    for text in ("a", "é", "€", "\U0001F600", "\x7f", "\x00"):
        assert r.matches(text.encode()), text
    for raw in (b"\n", b"\xc3", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80", b"\x80", b"ab"):
        assert not r.matches(raw), raw
    n = K.Regex(r"[^a]")
    assert n.matches(b"\n") and n.matches("é".encode()) and not n.matches(b"a") and not n.matches(b"\xc3")


# ---- 4. the flags by graph search ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", list(CC.PATTERNS) + [K.json_string(), K.json_object({"a": K.integer(), "b": K.json_string()}), K.number()])
def test_flags_by_graph_search(pattern):
    r = K.Regex(pattern)
    assert r.start == 0 and r.trans.shape == (r.states, 256) and 1 <= r.states <= K.MAX_STATES
    assert ((r.trans == CC.DEAD) | (r.trans < r.states)).all()
    live, closed = CC.flags_by_search(r.trans, r.accepting)
    assert live.all(), "the table holds a state that cannot reach an accepting state"
    assert (closed == r.closed.astype(bool)).all()
    reached = {0}
    todo = [0]
    while todo:
        q = todo.pop()
        for t in set(r.trans[q].tolist()) - {CC.DEAD}:
            if t not in reached:
                reached.add(t)
                todo.append(t)
    assert len(reached) == r.states, "the table holds a state the start state cannot reach"


def test_the_table_is_minimal_on_known_languages():
    assert K.Regex(r"(a|b)*abb").states == 4
    assert K.Regex(r"a{255}").states == 256
    assert K.Regex(r"(?:yes|no)").states == 5        # start, y, ye, n, and one closed end
    assert K.Regex(r"[ab]*a[ab]{3}").states == 16


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------

REFUSED = [
    (r"a*?", "lazy quantifier", 2), (r"a+?", "lazy quantifier", 2), (r"a??", "lazy quantifier", 2), (r"a{1,2}?", "lazy quantifier", 6),
    (r"a*+", "possessive quantifier", 2), (r"^a", "anchor ^", 0), (r"a$", "anchor $", 1), (r"\Aa", r"anchor \A", 0), (r"a\Z", r"anchor \Z", 1),
    (r"a\b", r"anchor \b", 1), (r"\Ba", r"anchor \B", 0), (r"(a)\1", "back-reference", 3), (r"(?=a)b", "look-ahead", 0),
    (r"(?!a)b", "look-ahead", 0), (r"(?<=a)b", "look-behind", 0), (r"(?<!a)b", "look-behind", 0), (r"(?P<n>a)", "named group", 0),
    (r"(?i)a", "inline flags", 0), (r"(?#x)a", "comment group", 0), (r"\D", r"negated shorthand \D", 0), (r"\W", r"negated shorthand \W", 0),
    (r"\S", r"negated shorthand \S", 0), (r"[é]", "non-ASCII class member", 1), (r"[a\xe9]", "non-ASCII class member", 2),
    (r"a{256}", "repeat count above 255", 1), (r"a{1,256}", "repeat count above 255", 1), (r"a{3,2}", "m > n", 1), (r"a{,3}", "unsupported construct {", 1),
    (r"a{", "unsupported construct {", 1), (r"{2}", "unsupported construct {", 0), (r"*a", "nothing to repeat", 0), (r"a|+", "nothing to repeat", 2),
    (r"a**", "multiple repeat", 2), (r"a{2}{3}", "multiple repeat", 4), (r"(a", "missing )", 0), (r"a)", "unbalanced )", 1),
    (r"[a", "unterminated character class", 0), (r"[z-a]", "bad character range", 1), (r"[\d-z]", "bad character range", 1),
    ("a\\", "trailing backslash", 1), (r"\x4", r"\x needs two hex digits", 0), (r"\q", "unknown escape", 0), (r"\u00e9", "unicode escape", 0),
    (r"\0", "octal escape", 0), ("(" * 65 + "a" + ")" * 65, "nested deeper than 64", 64),
]


@pytest.mark.parametrize("pattern,what,offset", REFUSED)
def test_refused_constructs_name_the_construct_and_its_offset(pattern, what, offset):
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Regex(pattern)
    assert e.value.code == E.INVALID_CONFIG
    assert what in str(e.value) and f"at offset {offset}" in str(e.value), str(e.value)


def test_invalid_utf8_in_the_pattern_is_refused():
    h = C.c_void_p()
    assert kjarni_amd.lib().kjarni_hip_regex_compile(b"a\xc3(", C.byref(h)) == E.INVALID_CONFIG
    assert "invalid UTF-8" in _ffi.last_error() and "offset 1" in _ffi.last_error()


def test_the_state_cap_gives_the_count():
    assert K.Regex(r"[ab]*a[ab]{11}").states == 4096              # exactly the cap
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Regex(r"[ab]*a[ab]{12}")
    assert e.value.code == E.INVALID_CONFIG and "8192 states" in str(e.value) and "4096" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:           # a pattern whose expansion alone is too large
        K.Regex(r"(?:(?:(?:a{255}){255}){255}){255}")
    assert e.value.code == E.INVALID_CONFIG and "states" in str(e.value)


def test_no_accepted_syntax_has_an_empty_language():
    """Without anchors and look-around every atom of the syntax matches something (a class cannot be empty, a negated class
    always matches the non-ASCII scalars), so the compiler's empty-language refusal cannot be reached from a pattern; the nearest
    things are the languages that hold the empty string alone."""
    for pattern in ("", "()", "a{0}", "(?:)*", "|"):
        r = K.Regex(pattern)
        assert r.states == 1 and r.accepting[0] and r.closed[0]
    assert K.Regex(r"[^\x00-\x7f]").matches("é".encode())


# ---- 6. token bytes -----------------------------------------------------------------------------------------------------------------

def _gpt2_byte_map():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def test_token_bytes_of_a_byte_level_table(tmp_path):
    m = _gpt2_byte_map()
    enc = lambda raw: "".join(m[b] for b in raw)  # noqa: E731
    pieces = [bytes([b]) for b in range(256)] + [b" the", b"\n\n", "é".encode(), b"\xc3\xc3", b"  x", b"\x00\xff"]
    vocab = {enc(p): i for i, p in enumerate(pieces)}
    n = len(pieces)
    tok = {"version": "1.0", "truncation": None, "padding": None,
           "added_tokens": [{"id": n, "content": "<|endoftext|>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                             "special": True},
                            {"id": n + 1, "content": "<tool>", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True,
                             "special": False}],
           "normalizer": None, "pre_tokenizer": {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True},
           "post_processor": None, "decoder": {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True},
           "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": "", "end_of_word_suffix": "",
                     "fuse_unk": False, "byte_fallback": False, "vocab": vocab, "merges": []}}
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(tok, ensure_ascii=False), encoding="utf-8")
    t = kjarni_amd.BpeTokenizer(str(path))
    for i, p in enumerate(pieces):
        assert t.token_bytes(i) == p, i
    assert t.token_bytes(n) == b"" and t.token_bytes(n + 1) == b""         # special and added: no bytes
    assert t.token_bytes(n + 2) == b"" and t.token_bytes(10 ** 6) == b""   # not in the file


def test_token_bytes_of_the_fixture_tokenizers():
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    t = kjarni_amd.BpeTokenizer(os.path.join(golden, "bpe_gpt2_tokenizer.json"))
    text = "The quick brown fox, naïve café: 12.5 €\n"
    ids = t.encode(text)
    assert b"".join(t.token_bytes(i) for i in ids) == text.encode()
    assert t.token_bytes(700) == b""                                       # <|endoftext|>
    sp = kjarni_amd.BpeTokenizer(os.path.join(golden, "spbpe_legacy_tokenizer.json"))
    vocab = json.load(open(os.path.join(golden, "spbpe_legacy_tokenizer.json"), encoding="utf-8"))["model"]["vocab"]
    added = {a["id"] for a in json.load(open(os.path.join(golden, "spbpe_legacy_tokenizer.json"), encoding="utf-8"))["added_tokens"]}
    seen_byte = seen_space = False
    for piece, i in vocab.items():
        got = sp.token_bytes(i)
        if i in added:
            assert got == b"", piece
        elif re.fullmatch(r"<0x[0-9A-F]{2}>", piece):
            assert got == bytes([int(piece[3:5], 16)]), piece
            seen_byte = True
        else:
            assert got == piece.replace("▁", " ").encode(), piece
            seen_space = seen_space or "▁" in piece
    assert seen_byte and seen_space
    ids = sp.encode("Hello wörld")
    assert b"".join(sp.token_bytes(i) for i in ids).lstrip(b" ") == "Hello wörld".encode()


# ---- 7. the builders ------------------------------------------------------------------------------------------------------------------

def _accepts(pattern, yes, no):
    r = K.Regex(pattern)
    for t in yes:
        assert re.fullmatch(pattern, t, re.ASCII), (pattern, t)
        assert r.matches(t.encode()), (pattern, t)
    for t in no:
        assert not re.fullmatch(pattern, t, re.ASCII), (pattern, t)
        assert not r.matches(t.encode()), (pattern, t)
    return r


def test_choices():
    opts = ["yes", "no", "a|b", "x.y", "(z)", "né", "{}", "q\"t", "tab\there", "[1]*"]
    r = _accepts(K.choices(opts), opts, ["", "ye", "yesno", "a", "b", "xzy", "z", "tabthere", "1"])
    for o in opts:
        assert r.closed[r.step(r.start, o.encode())] or any(p != o and p.startswith(o) for p in opts)
    with pytest.raises(ValueError):
        K.choices([])


def test_integer_and_number():
    _accepts(K.integer(), ["0", "-0", "7", "-12", "1000"], ["", "-", "01", "+1", "1.0", "1e3", " 1"])
    yes = ["0", "-0.5", "12.25", "1e5", "1E-5", "3.0e+10", "-7"]
    _accepts(K.number(), yes, ["", ".5", "1.", "01.5", "1e", "1e+", "--1", "0x1", "NaN"])
    for t in yes:
        assert isinstance(json.loads(t), (int, float))


def test_json_string():
    yes = ['""', '"a"', '"hello world"', '"café €"', r'"a\"b"', r'"\\"', r'"\n\t\r\b\f\/"', r'"éꯍ"', '"{}[],:"']
    no = ['', '"', '"a', 'a"', '"a"b"', '"\n"', '"\t"', r'"\q"', r'"\u12"', r'"\"', "'a'", '"\x1f"']
    _accepts(K.json_string(), yes, no)
    for t in yes:
        assert isinstance(json.loads(t), str)


def test_json_object():
    pattern = K.json_object({"name": K.json_string(), "age": K.integer(), "score": K.number(), "ok": K.choices(["true", "false"]),
                             "k\"ey é": K.choices(["null"])})
    yes = ['{"name":"Ada","age":36,"score":1.5e3,"ok":true,"k\\"ey é":null}', '{"name":"","age":-1,"score":0,"ok":false,"k\\"ey é":null}']
    no = ['{}', '{"name":"Ada"}', '{"age":36,"name":"Ada","score":1,"ok":true,"k\\"ey é":null}',
          '{"name": "Ada","age":36,"score":1,"ok":true,"k\\"ey é":null}', '{"name":"Ada","age":36,"score":1,"ok":true,"k\\"ey é":null} ']
    r = _accepts(pattern, yes, no)
    for t in yes:
        obj = json.loads(t)
        assert list(obj) == ["name", "age", "score", "ok", "k\"ey é"]
    assert r.closed[r.step(r.start, yes[0].encode())]              # nothing follows the closing brace
    _accepts(K.json_object({}), ["{}"], ["", "{ }", "{"])
    # samples drawn from the automaton itself parse as JSON and match re
    rng = np.random.default_rng(5)
    for _ in range(50):
        q, out = r.start, bytearray()
        while not r.closed[q]:
            nxt = [b for b in range(0x20, 0x100) if r.trans[q, b] != CC.DEAD]   # (the table admits well-formed UTF-8 only)
            b = int(nxt[rng.integers(0, len(nxt))]) if len(out) < 150 else min(nxt, key=lambda c: _to_end(r, int(r.trans[q, c])))
            out.append(b)
            q = int(r.trans[q, b])
        text = bytes(out).decode()
        assert re.fullmatch(pattern, text, re.ASCII), text
        assert list(json.loads(text)) == ["name", "age", "score", "ok", "k\"ey é"]


_DIST = {}


def _to_end(r, q):
    """Fewest bytes from q to a closed state."""
    key = id(r)
    if key not in _DIST:
        dist = np.where(r.closed.astype(bool), 0, 10 ** 6)
        for _ in range(r.states):
            for s in range(r.states):
                nxt = [dist[t] for t in r.trans[s] if t != CC.DEAD]
                if nxt:
                    dist[s] = min(dist[s], 1 + min(nxt))
        _DIST[key] = dist
    return int(_DIST[key][q])


def test_escape_round_trips():
    for text in ["a.b", "1+1=2?", "x|y", "(a)[b]{c}", "back\\slash", "q\"t", "line\nbreak\ttab\r", "café €", "^$*-,: ~#&"]:
        _accepts(K.escape(text), [text], [text + "x", text[:-1]])
