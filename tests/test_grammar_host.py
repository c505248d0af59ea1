"""Grammar-constrained decoding, host side (no GPU): the new symbols, their arities and what they do with NULL; the compiled
stack automaton against an independent recogniser over enumerated strings; json_value against json.loads and json_schema against
a validator of the subset; every refusal of the compiler from a minimal grammar, with the rule named; the limits; the depth
rule; kjarni_hip_grammar_walk against the table walker of tests/grammar_cases.py."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi
from kjarni_amd import constraints as K
from kjarni_amd._ffi import KjarniError as E
from tests import grammar_cases as GC

SYMBOLS = {
    "kjarni_hip_grammar_compile": 4, "kjarni_hip_grammar_free": 1, "kjarni_hip_grammar_dims": 3, "kjarni_hip_grammar_table": 4,
    "kjarni_hip_grammar_walk": 11, "kjarni_hip_grammar_constraint_new": 6, "kjarni_hip_grammar_constraint_free": 1,
    "kjarni_hip_grammar_constraint_dims": 3, "kjarni_hip_op_grammar_apply": 12, "kjarni_hip_op_grammar_advance": 15,
    "kjarni_hip_decoder_generate_grammar": 11, "kjarni_hip_generator_set_grammar": 4, "kjarni_hip_chat_set_grammar": 4,
    "kjarni_hip_generator_grammar_result": 2, "kjarni_hip_chat_grammar_result": 2,
}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kjarni_hip.h")


# ---- 1. symbols and NULL behaviour ---------------------------------------------------------------------------------------------------

def test_symbols_and_arities():
    L = kjarni_amd.lib()
    for name, argc in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(_ffi.SIGNATURES[name][1]) == argc, name
    assert callable(kjarni_amd.HipDecoder.generate_grammar)
    assert callable(kjarni_amd.Generator.set_grammar) and callable(kjarni_amd.Chat.set_grammar)
    for name in ("json_value", "json_schema", "Grammar", "GrammarConstraint"):
        assert callable(getattr(K, name))


def test_the_header_declares_what_ffi_mirrors():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, argc in SYMBOLS.items():
        m = re.search(r"\b(\w[\w\s\*]*?)\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in kjarni_hip.h"
        assert len([a for a in m.group(2).split(",") if a.strip()]) == argc, name
        assert (_ffi.SIGNATURES[name][0] is C.c_int32) == ("KjarniErrorCode" in m.group(1)), name
    for macro, value in (("MAX_RULES", 256), ("MAX_STATES", 4096), ("MAX_DEPTH", 64), ("TOKEN_PUSHES", 16)):
        assert re.search(r"#define\s+KJARNI_GRAMMAR_%s\s+%d\b" % (macro, value), text)
        assert getattr(K, "GRAMMAR_" + macro) == value
    assert (GC.MAX_DEPTH, GC.TOKEN_PUSHES) == (K.GRAMMAR_MAX_DEPTH, K.GRAMMAR_TOKEN_PUSHES)
    fields = [f for f, _ in _ffi.KjarniHipGrammarResult._fields_]
    assert fields == ["final_state", "device_state", "final_depth", "device_depth", "accepted", "complete", "violated"]
    m = re.search(r"typedef struct KjarniHipGrammarResult \{(.*?)\}", text, re.S)
    assert [w for w in re.findall(r"\w+", m.group(1)) if w in fields] == fields
    # the grammar block stands behind the constraint block, and the regex compiler's surface is as it was
    assert text.index("kjarni_hip_chat_constraint_result") < text.index("KJARNI_GRAMMAR_MAX_RULES")


def test_null_arguments():
    L = kjarni_amd.lib()
    h = C.c_void_p()
    names, pats = (C.c_char_p * 1)(b"s"), (C.c_char_p * 1)(b"a")
    assert L.kjarni_hip_grammar_compile(None, pats, 1, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_compile(names, None, 1, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_compile(names, pats, 1, None) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_compile((C.c_char_p * 1)(None), pats, 1, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_compile(names, pats, 0, C.byref(h)) == E.INVALID_CONFIG and not h.value
    L.kjarni_hip_grammar_free(None)
    L.kjarni_hip_grammar_constraint_free(None)
    assert L.kjarni_hip_grammar_dims(None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_table(None, None, None, None) == E.NULL_POINTER
    g = K.Grammar([("s", "a(?&s)?b")])
    assert L.kjarni_hip_grammar_dims(g._h, None, None) == E.OK
    assert L.kjarni_hip_grammar_table(g._h, None, None, None) == E.OK
    q, d, alive = C.c_uint32(77), C.c_int32(77), C.c_int32(77)
    st = (C.c_uint16 * 64)()
    assert L.kjarni_hip_grammar_walk(None, 0, None, 0, None, 0, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_walk(g._h, 0, None, 0, None, 0, 0, None, st, C.byref(d), C.byref(alive)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_walk(g._h, 0, None, 0, None, 2, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_walk(g._h, 0, None, 1, None, 0, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.NULL_POINTER
    assert (q.value, d.value, alive.value) == (77, 77, 77)
    assert L.kjarni_hip_grammar_walk(g._h, 0, None, 0, None, 0, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.OK
    assert (q.value, d.value, alive.value) == (0, 0, 1)
    # no such state, a depth out of range: not alive, the outputs left alone
    q.value = 77
    assert L.kjarni_hip_grammar_walk(g._h, 9999, None, 0, None, 0, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.OK
    assert alive.value == 0 and q.value == 77
    assert L.kjarni_hip_grammar_walk(g._h, 0, st, 65, None, 0, 0, C.byref(q), st, C.byref(d), C.byref(alive)) == E.OK and alive.value == 0
    off = np.zeros(3, np.uint32)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    assert L.kjarni_hip_grammar_constraint_new(0, None, u32(off), None, 2, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_constraint_new(0, g._h, None, None, 2, C.byref(h)) == E.NULL_POINTER
    assert L.kjarni_hip_grammar_constraint_new(0, g._h, u32(off), None, 2, None) == E.NULL_POINTER
    # a malformed table is refused before any GPU work (so: here, without a GPU)
    bad = np.array([0, 2, 1], np.uint32)
    assert L.kjarni_hip_grammar_constraint_new(0, g._h, u32(bad), (C.c_uint8 * 2)(97, 98), 2, C.byref(h)) == E.INVALID_CONFIG
    assert "decreases" in _ffi.last_error()
    assert L.kjarni_hip_grammar_constraint_new(0, g._h, u32(np.array([0, 1, 2], np.uint32)), None, 2, C.byref(h)) == E.INVALID_CONFIG
    assert L.kjarni_hip_grammar_constraint_new(0, g._h, u32(np.array([1, 1, 2], np.uint32)), (C.c_uint8 * 2)(97, 98), 2, C.byref(h)) == E.INVALID_CONFIG
    assert L.kjarni_hip_grammar_constraint_dims(None, None, None) == E.NULL_POINTER
    assert L.kjarni_hip_generator_set_grammar(None, names, pats, 1) == E.NULL_POINTER
    assert L.kjarni_hip_chat_set_grammar(None, None, None, 0) == E.NULL_POINTER
    res = _ffi.KjarniHipGrammarResult(9, 9, 9, 9, 9, 9, 9)
    assert L.kjarni_hip_generator_grammar_result(None, C.byref(res)) == E.NULL_POINTER
    assert L.kjarni_hip_chat_grammar_result(None, None) == E.NULL_POINTER


def test_op_hooks_check_their_arguments_without_a_device():
    L = kjarni_amd.lib()
    logits = np.full(4, 7.0, np.float32)
    out = np.full(4, 9.0, np.float32)
    f32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert L.kjarni_hip_op_grammar_apply(0, None, f32(logits), 1, 4, None, None, None, None, None, 0, f32(out)) == E.NULL_POINTER
    assert (out == 9.0).all()
    v = np.full(1, 9, np.int32)
    assert L.kjarni_hip_op_grammar_advance(0, None, None, 1, None, None, None, None, None, 0, v.ctypes.data_as(C.POINTER(C.c_int32)), 0, 0, None,
                                           None) == E.NULL_POINTER
    assert v[0] == 9
    o = _ffi.KjarniHipSamplingOptions()
    o.max_new_tokens, o.repetition_penalty = 4, 1.0
    p, ids, cnt = np.array([5, 6, 7], np.uint32), np.zeros(4, np.uint32), C.c_size_t(7)
    u32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    cb = _ffi.KjarniTokenCallbackFn()
    res = _ffi.KjarniHipGrammarResult(9, 9, 9, 9, 9, 9, 9)
    gen = L.kjarni_hip_decoder_generate_grammar
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(ids), 4, C.byref(cnt), C.byref(res)) == E.NULL_POINTER
    assert cnt.value == 0 and (res.final_state, res.final_depth, res.accepted, res.complete, res.violated) == (0, 0, 0, 0, 0)
    assert gen(None, None, u32(p), 3, None, cb, None, u32(ids), 4, C.byref(cnt), None) == E.NULL_POINTER
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(ids), 4, None, None) == E.NULL_POINTER
    u = np.zeros(2, np.float32)
    o.uniforms, o.n_uniforms = u.ctypes.data_as(C.POINTER(C.c_float)), 2          # judged ahead of the handles
    assert gen(None, None, u32(p), 3, C.byref(o), cb, None, u32(ids), 4, C.byref(cnt), None) == E.INVALID_CONFIG


# ---- 2. the compiled machine against the independent recogniser -------------------------------------------------------------------------

def _strings(alphabet, bound):
    for n in range(bound + 1):
        for tup in itertools.product(alphabet, repeat=n):
            yield "".join(tup).encode()


@pytest.mark.parametrize("name", list(GC.TREES))
def test_compiled_grammar_against_the_recogniser(name):
    tree, alphabet, bound = GC.TREES[name]
    g = K.Grammar(GC.rules_of(tree))
    matched = 0
    for data in _strings(alphabet, bound):
        want = GC.matches(tree, data)
        c = GC.walk(g.action, g.flags, GC.START, data)
        assert GC.accepted(g.flags, c) == want, (name, data)
        matched += want
    assert matched >= 3, "precondition: the bound admits too few matches"
    if name == "flat":   # no call at all: the verdicts of the pattern compiler on the same strings, and no stack anywhere
        r = K.Regex(GC.rules_of(tree)[0][1])
        assert not ((g.action >> 30) == 2).any()
        for data in _strings(alphabet, bound):
            assert g.matches(data) == r.matches(data), data
            c = GC.walk(g.action, g.flags, GC.START, data)
            assert (c is None) == (r.step(r.start, data) == K.DEAD), data


def test_the_table_says_what_the_header_says():
    g = K.Grammar(GC.rules_of(GC.CHAIN))
    assert g.kept_rules == 4 and g.rule_of[0] == 0
    kinds = g.action >> 30
    assert set(np.unique(kinds)) <= {0, 1, 2}
    assert (g.action[kinds == 0] == 0).all()
    nxt, ret = g.action & 0xFFF, (g.action >> 12) & 0xFFF
    assert (nxt[kinds > 0] < g.states).all() and (ret[kinds == 2] < g.states).all()
    for q in range(g.states):
        assert bool(g.flags[q] & 2) == (not (kinds[q] > 0).any())
        assert (g.rule_of[nxt[q][kinds[q] == 1]] == g.rule_of[q]).all()           # a move stays in its rule
        assert (g.rule_of[ret[q][kinds[q] == 2]] == g.rule_of[q]).all()           # a call returns into its rule
    # one byte, three calls deep: x at the start pushes a's, b's and c's return states
    c = GC.walk(g.action, g.flags, GC.START, b"x")
    assert c is not None and len(c[1]) == 3 and [int(g.rule_of[s]) for s in c[1]] == [0, 1, 2] and g.rule_of[c[0]] == 3
    assert g.walk(GC.START, b"x") == c and g.matches(b"xyuvw") and not g.matches(b"xyuv")
    # a rule rule 0 never reaches is dropped silently -- unless its pattern is refused on its own
    assert K.Grammar([("s", "a"), ("unused", "(?&s)b")]).kept_rules == 1


_MUTANTS = b"{}[]\",:\\ 0e-.1t"


# ---- 3. json_value against json.loads ------------------------------------------------------------------------------------------------

def test_json_value_on_enumerated_strings():
    compact, spaced = K.Grammar(K.json_value()), K.Grammar(K.json_value(whitespace=True))
    assert [n for n, _ in K.json_value()] == ["value", "object", "array"]
    assert [n for n, _ in K.json_value(True)] == ["json", "value", "object", "array"]
    accepted = 0
    for data in _strings("{}[]\",:0-9tfn\\ ", 4):
        ok, _, text = GC.parse(data)
        assert spaced.matches(data) == ok, data
        assert compact.matches(data) == (ok and GC.no_space_outside_strings(text)), data
        accepted += ok
    assert accepted > 100
    for text in ("true", "false", "null", "[true,false,null]", "{\"a\":{\"b\":[1.5e-3,-0,\"\\u00e9\\n\"]}}", "\"é€😀\""):
        assert compact.matches(text.encode()) and spaced.matches(text.encode()), text
    for text in ("tru", "nul", "[1,]", "{\"a\":}", "{a:1}", "01", "1.", "\"\\x\"", "\"\n\"", "[1 2]", "{\"a\":1,}", "\xff"):
        assert not spaced.matches(text.encode("latin1") if text == "\xff" else text.encode()), text


def test_json_value_on_random_documents_and_their_mutations():
    compact, spaced = K.Grammar(K.json_value()), K.Grammar(K.json_value(whitespace=True))
    rng = np.random.default_rng(5)
    flipped_to_invalid = 0
    for k in range(150):
        doc = GC.random_document(rng)
        tight = json.dumps(doc, ensure_ascii=bool(k % 2), separators=(",", ":")).encode()
        loose = json.dumps(doc, ensure_ascii=False, indent=int(k % 3) or None).encode()
        assert compact.matches(tight) and spaced.matches(tight), tight
        assert spaced.matches(loose), loose
        for _ in range(6):
            m = bytearray(tight)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 256)) if rng.integers(0, 2) else _MUTANTS[int(rng.integers(0, len(_MUTANTS)))]
            ok, _, text = GC.parse(bytes(m))
            assert spaced.matches(bytes(m)) == ok, bytes(m)
            assert compact.matches(bytes(m)) == (ok and GC.no_space_outside_strings(text)), bytes(m)
            flipped_to_invalid += not ok
    assert flipped_to_invalid > 100


# ---- 4. json_schema against the validator ------------------------------------------------------------------------------------------------

_POINT = {"type": "object", "properties": {"x": {"type": "number"}, "y": {"type": "number"}}, "required": ["x", "y"]}
SCHEMAS = {
    "scalars": {"type": "object", "properties": {"s": {"type": "string"}, "i": {"type": "integer"}, "n": {"type": "number"}, "b": {"type": "boolean"},
                                                 "z": {"type": "null"}}, "required": ["s", "i", "n", "b", "z"]},
    "nested": {"type": "object", "properties": {"a": _POINT, "b": {"type": "object", "properties": {"c": _POINT}, "required": ["c"]}},
               "required": ["a", "b"], "title": "ignored", "description": "ignored"},
    "optional_first": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}},
                       "required": ["b", "c"]},
    "optional_middle": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}},
                        "required": ["a", "c"]},
    "optional_last": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}},
                      "required": ["a", "b"]},
    "optional_all": {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "string"}, "c": {"type": "boolean"}}},
    "array_of_objects": {"type": "array", "items": _POINT, "minItems": 1, "maxItems": 3},
    "any_of": {"anyOf": [{"type": "integer"}, {"type": "string"}, {"type": "array", "items": {"type": "boolean"}}, _POINT]},
    "enum_const": {"type": "object", "properties": {"kind": {"enum": ["a", "b c", 3, None, True]}, "v": {"const": "é\"x"}}, "required": ["kind"]},
    "type_list": {"type": "array", "items": {"type": ["integer", "null", "string"]}, "maxItems": 4},
    "tree": {"type": "object", "properties": {"value": {"type": "integer"}, "kids": {"type": "array", "items": {"$ref": "#"}}},
             "required": ["value"]},
    "defs": {"$defs": {"leaf": {"type": "object", "properties": {"n": {"type": "integer"}}, "required": ["n"]},
                       "node": {"type": "object", "properties": {"l": {"anyOf": [{"$ref": "#/$defs/leaf"}, {"type": "null"}]},
                                                                 "r": {"$ref": "#/$defs/node"}}, "required": ["l"]}},
             "$ref": "#/$defs/node"},
    "free_form": {"type": "object", "properties": {"name": {"type": "string"}, "arguments": {}, "extra": True}, "required": ["name", "arguments"]},
}


@pytest.mark.parametrize("name", list(SCHEMAS))
def test_json_schema_against_the_validator(name):
    schema = SCHEMAS[name]
    compact, spaced = K.Grammar(K.json_schema(schema)), K.Grammar(K.json_schema(schema, whitespace=True))
    rng = np.random.default_rng(len(name))
    rejected = 0
    for k in range(40):
        doc = GC.random_instance(schema, rng)
        tight = json.dumps(doc, ensure_ascii=False, separators=(",", ":")).encode()
        ok, value, _ = GC.parse(tight)
        assert ok and GC.valid(schema, value), (name, tight)        # (the generator and the validator agree)
        assert compact.matches(tight) and spaced.matches(tight), (name, tight)
        assert spaced.matches(json.dumps(doc, ensure_ascii=False, indent=1).encode()), (name, doc)
        for _ in range(8):
            m = bytearray(tight)
            m[int(rng.integers(0, len(m)))] = int(rng.integers(32, 127)) if rng.integers(0, 3) else _MUTANTS[int(rng.integers(0, len(_MUTANTS)))]
            ok, value, text = GC.parse(bytes(m))
            want = ok and GC.valid(schema, value)
            assert spaced.matches(bytes(m)) == want, (name, bytes(m))
            assert compact.matches(bytes(m)) == (want and GC.no_space_outside_strings(text)), (name, bytes(m))
            rejected += not want
    assert rejected > 40
    # a random document of any shape is judged as the validator judges it
    for k in range(30):
        tight = json.dumps(GC.random_document(rng), ensure_ascii=False, separators=(",", ":")).encode()
        ok, value, _ = GC.parse(tight)
        assert compact.matches(tight) == GC.valid(schema, value), (name, tight)


def test_json_schema_refuses_what_it_does_not_build():
    for schema, word in (({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "object", "patternProperties": {}}, "patternProperties"),
                         ({"allOf": [{"type": "string"}]}, "allOf"), ({"not": {}}, "not"), ({"type": "string", "format": "date"}, "format"),
                         ({"type": "integer", "minimum": 0}, "minimum"), ({"type": "object", "additionalProperties": {"type": "string"}}, "additionalProperties"),
                         ({"type": "array", "maxItems": 256}, "maxItems"), ({"$ref": "other.json"}, "$ref"), ({"enum": [[1]]}, "scalars"),
                         ({"type": "tuple"}, "tuple")):
        with pytest.raises(ValueError) as e:
            K.json_schema(schema)
        assert word in str(e.value), schema
    # a conflict between alternatives is the compiler's refusal, passed on: both start with a digit
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Grammar(K.json_schema({"anyOf": [{"type": "integer"}, {"$ref": "#/$defs/n"}], "$defs": {"n": {"type": "number"}}}))
    assert e.value.code == E.INVALID_CONFIG and "two ways to continue" in str(e.value)


# ---- 5. refusals and limits ------------------------------------------------------------------------------------------------------------

REFUSALS = [
    ([("s", "a|(?&t)"), ("t", "ab")], ["'s'", "two ways to continue", "0x61", "'t'", "byte edge"]),
    ([("s", "(?&t)|(?&u)"), ("t", "ab"), ("u", "ac")], ["'s'", "two ways to continue", "0x61", "another called rule"]),
    ([("s", "a(?&t)b"), ("t", "b+")], ["'t'", "may either end or go on", "0x62"]),
    ([("s", "x(?&t)y"), ("t", "(?&u)"), ("u", "ay*")], ["'u'", "may either end or go on", "0x79"]),      # FOLLOW through t's accepting return state
    ([("s", "a(?&t)c"), ("t", "b*")], ["'t'", "matches the empty string", "'s'"]),
    ([("s", "(?&s)a|a")], ["'s'", "left recursion"]),
    ([("s", "(?&t)"), ("t", "(?&u)x|y"), ("u", "(?&s)z")], ["left recursion"]),
    ([("s", "a(?&s)")], ["'s'", "no finite string"]),
    ([("s", "a|b(?&t)"), ("t", "c(?&t)")], ["'t'", "no finite string"]),
    ([("s", "a(?&nope)")], ["'s'", "undefined", "'nope'"]),
    ([("s", "a"), ("s", "b")], ["'s'", "twice"]),
    ([("9s", "a")], ["bad rule name"]),
    ([("s-t", "a")], ["bad rule name"]),
    ([("s", "(?&9t)")], ["'s'", "malformed rule call", "offset 0"]),
    ([("s", "a(?&t")], ["'s'", "malformed rule call", "offset 1"]),
    ([("s", "x"), ("t", "a*?")], ["'t'", "lazy quantifier", "offset 2"]),                                 # per-pattern refusals, in an unreached rule too
    ([("s", "^a")], ["'s'", "unsupported anchor ^", "offset 0"]),
    ([("s", "(?P<n>a)")], ["'s'", "named group"]),
    ([("s", "a{256}")], ["'s'", "repeat count above 255"]),
]


@pytest.mark.parametrize("rules,words", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_every_refusal_names_its_rule(rules, words):
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Grammar(rules)
    assert e.value.code == E.INVALID_CONFIG
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_the_regex_compiler_keeps_refusing_the_call():
    for pattern in ("(?&s)", "a(?&s)b"):
        with pytest.raises(kjarni_amd.KjarniException) as e:
            K.Regex(pattern)
        assert e.value.code == E.INVALID_CONFIG and "unsupported" in str(e.value)


def test_limits():
    chain = [("r%d" % i, "a" if i == 255 else "(?&r%d)" % (i + 1)) for i in range(256)]
    g = K.Grammar(chain)                                           # 256 rules are fine (and a chain of 255 first calls on one byte)
    assert g.kept_rules == 256 and g.walk(GC.START, b"a") is None  # ... though it needs 255 calls open at once: deeper than 64
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Grammar([("r%d" % i, "a") for i in range(257)])
    assert "257" in str(e.value) and "256" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Grammar([("s", "(?&t)x"), ("t", "[ab]*a[ab]{12}")])      # 2^13 subset states in t
    assert re.search(r"\b8\d\d\d states", str(e.value)) and "4096" in str(e.value)
    with pytest.raises(kjarni_amd.KjarniException) as e:
        K.Grammar([("s", "[ab]*a[ab]{14}")])                       # past the bound on one rule's subset construction
    assert "'s'" in str(e.value) and "states" in str(e.value)


def test_depth_counts_calls_not_brackets():
    """The limit is on calls open at once, not on brackets.  In top := (?&v), v := [0-9]+|\\[(?:(?&v)(?:,(?&v))*)?\\] every value
    is one call, so 64 nested [ are a live prefix with 64 calls open, and the 65th [ dies (as does a digit there: a value too).
    The same v as rule 0 has its outermost value for free: 65 [ live, the 66th dies.  In json_value a container inside a
    container costs two calls (value, then object or array) and the outermost value none: 32 levels of nesting hold 63 calls and
    are accepted, a 33rd level would need 65."""
    tree = [("top", GC.Call("v"))] + GC.LISTS
    g = K.Grammar(GC.rules_of(tree))
    c = g.walk(GC.START, b"[" * 64)
    assert c is not None and len(c[1]) == 64
    assert g.walk(GC.START, b"[" * 65) is None and g.walk(c, b"[") is None
    assert g.walk(c, b"1") is None and g.walk(c, b"]") is not None
    assert g.matches(b"[" * 64 + b"]" * 64) and not g.matches(b"[" * 65 + b"]" * 65)
    assert GC.matches(tree, b"[" * 64 + b"]" * 64, max_depth=64) and not GC.matches(tree, b"[" * 65 + b"]" * 65, max_depth=64)
    assert GC.matches(tree, b"[" * 65 + b"]" * 65)                  # (the grammar itself has no limit)
    bare = K.Grammar(GC.rules_of(GC.LISTS))
    assert len(bare.walk(GC.START, b"[" * 65)[1]) == 64 and bare.walk(GC.START, b"[" * 66) is None
    j = K.Grammar(K.json_value())
    assert j.matches(b"[" * 32 + b"]" * 32) and j.matches(b"{\"a\":" * 31 + b"{}" + b"}" * 31)
    assert not j.matches(b"[" * 33 + b"]" * 33)
    deep = j.walk(GC.START, b"[" * 32)
    assert deep is not None and len(deep[1]) == 63
    assert j.walk(deep, b"1") is not None and j.walk(deep, b"]") is not None and j.walk(deep, b"[") is None


# ---- 6. the exported walk against the table walker ------------------------------------------------------------------------------------

def test_the_exported_walk_against_the_table_walker():
    rng = np.random.default_rng(3)
    for rules, alphabet, deep in ((K.json_value(), b"{}[]\",:01a \\tn", b"[[{\"a\":["), (GC.rules_of(GC.BRACKETS), b"()[]", b"([(["),
                                  (GC.rules_of(GC.CHAIN), b"xyuvw", b"x")):
        g = K.Grammar(rules)
        configs = [GC.START] + [GC.walk(g.action, g.flags, GC.START, deep[:n]) for n in range(1, len(deep) + 1)]
        assert None not in configs
        for _ in range(400):
            c = configs[int(rng.integers(0, len(configs)))]
            data = bytes(alphabet[int(j)] for j in rng.integers(0, len(alphabet), int(rng.integers(0, 6))))
            for as_token in (False, True):
                want = GC.walk(g.action, g.flags, c, data, as_token)
                assert g.walk(c, data, as_token) == want, (c, data, as_token)
            if want is not None and len(configs) < 200:
                configs.append(want)
        assert max(len(c[1]) for c in configs) >= 3
    # the window: 16 own pushes live, the 17th dies as a token and lives as a string; pops give slots back
    g = K.Grammar(GC.rules_of([("top", GC.Call("v"))] + GC.LISTS))   # (every [ is one push)
    assert g.walk(GC.START, b"[" * 16, True) is not None and g.walk(GC.START, b"[" * 17, True) is None
    assert g.walk(GC.START, b"[" * 17, False) is not None
    busy = b"[" + b"[]," * 20 + b"[" * 15
    assert g.walk(GC.START, busy, True) is not None and g.walk(GC.START, busy + b"[", True) is None
    assert GC.own_pushes_peak(g.action, g.flags, GC.START, busy) == 16
    below = g.walk(GC.START, b"[" * 10)
    assert g.walk(below, b"]" * 10 + b"[" * 16, True) is None      # rule 0 ended: nothing follows
    assert g.walk(below, b"]" * 9 + b",[" + b"[" * 15, True) is not None and g.walk(below, b"]" * 9 + b",[" + b"[" * 16, True) is None
