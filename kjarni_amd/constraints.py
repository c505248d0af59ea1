"""Constrained decoding: patterns, the compiled DFA and the device constraint.

The string builders are pure Python and return patterns in the syntax the native compiler accepts (include/kjarni_hip.h:
kjarni_hip_regex_compile), with the meaning of Python's re.fullmatch(pattern, text, re.ASCII).  A regular expression cannot
count brackets, so the pattern builders are flat; nested and recursive formats are grammars: lists of rules (name, pattern) whose
patterns may call each other with (?&name) (kjarni_hip_grammar_compile), which json_value and json_schema build.

    Regex              a compiled pattern: the byte DFA (host only, no GPU)
    Constraint         a Regex and a token table with their mask on the device: what HipDecoder.generate_constrained takes
    Grammar            compiled rules: the stack automaton's action table, and its walk (host only, no GPU)
    GrammarConstraint  a Grammar and a token table on the device: what the two grammar kernels run on
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import check_error, lib

DEAD = 0xFFFF
MAX_STATES = 4096
MAX_STOPS = 16
GRAMMAR_MAX_RULES = 256
GRAMMAR_MAX_STATES = 4096
GRAMMAR_MAX_DEPTH = 64
GRAMMAR_TOKEN_PUSHES = 16

_META = set("\\.^$*+?{}[]()|\"")


def escape(text: str) -> str:
    """`text` as a literal of the pattern syntax (re.escape would also escape characters the compiler refuses to see escaped)."""
    out = []
    for ch in text:
        if ch in _META:
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\r":
            out.append("\\r")
        elif ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append("\\x%02x" % ord(ch))
        else:
            out.append(ch)
    return "".join(out)


def choices(options: Iterable[str]) -> str:
    """One of the given strings, exactly."""
    opts = list(options)
    if not opts:
        raise ValueError("choices() needs at least one option")
    return "(?:" + "|".join(escape(o) for o in opts) + ")"


def integer() -> str:
    """A JSON integer: optional minus, no leading zeros."""
    return "-?(?:0|[1-9][0-9]*)"


def number() -> str:
    """A JSON number: integer, optional fraction, optional exponent."""
    return integer() + "(?:\\.[0-9]+)?(?:[eE][+\\-]?[0-9]+)?"


def json_string() -> str:
    """A JSON string: no raw control characters, the two-character escapes and \\uXXXX."""
    return "\"(?:[^\"\\\\\\x00-\\x1f]|\\\\[\"\\\\/bfnrt]|\\\\u[0-9a-fA-F]{4})*\""


def json_object(fields: Mapping[str, str]) -> str:
    """A flat JSON object with these keys in this order, each value matching its pattern; minimal whitespace (none).
    json_object({"name": json_string(), "age": integer()}) matches {"name":"Ada","age":36}."""
    if not fields:
        return "\\{\\}"
    parts = ["\"" + escape(_json_key(k)) + "\":(?:" + v + ")" for k, v in fields.items()]
    return "\\{" + ",".join(parts) + "\\}"


def _json_key(key: str) -> str:
    import json
    return json.dumps(key, ensure_ascii=False)[1:-1]


class Regex:
    """A pattern compiled to a byte DFA (no GPU).  trans [states, 256] uint16 (DEAD = no move), start, accepting, closed."""

    def __init__(self, pattern: str):
        self._h = C.c_void_p()
        self.pattern = pattern
        check_error(lib().kjarni_hip_regex_compile(pattern.encode("utf-8"), C.byref(self._h)))
        n, start = C.c_int32(), C.c_uint32()
        check_error(lib().kjarni_hip_regex_dims(self._h, C.byref(n), C.byref(start)))
        self.states, self.start = int(n.value), int(start.value)
        self.trans = np.empty((self.states, 256), np.uint16)
        self.accepting = np.empty(self.states, np.uint8)
        self.closed = np.empty(self.states, np.uint8)
        check_error(lib().kjarni_hip_regex_table(self._h, self.trans.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                 self.accepting.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 self.closed.ctypes.data_as(C.POINTER(C.c_uint8))))

    def step(self, state: int, data: bytes) -> int:
        """The state after `data` from `state`; DEAD when the walk dies."""
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data.ljust(1, b"\0"))
        out = C.c_uint32()
        check_error(lib().kjarni_hip_regex_step(self._h, state, buf, len(data), C.byref(out)))
        return int(out.value)

    def matches(self, data: bytes) -> bool:
        q = self.step(self.start, data)
        return q != DEAD and bool(self.accepting[q])

    def close(self):
        if self._h:
            lib().kjarni_hip_regex_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def token_table(tokens: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """(tok_off [V + 1] uint32, tok_bytes uint8) of a vocabulary given as one bytes object per token."""
    off = np.zeros(len(tokens) + 1, np.uint32)
    off[1:] = np.cumsum([len(t) for t in tokens], dtype=np.uint64)
    data = np.frombuffer(b"".join(tokens), np.uint8).copy()
    return off, data


class Constraint:
    """A pattern (or a compiled Regex) and the vocabulary's token bytes, with the token mask built on the device."""

    def __init__(self, pattern, tokens: Sequence[bytes], device: int = 0):
        self.regex = pattern if isinstance(pattern, Regex) else Regex(pattern)
        self.tokens: List[bytes] = [bytes(t) for t in tokens]
        off, data = token_table(self.tokens)
        self._h = C.c_void_p()
        self.device = device
        check_error(lib().kjarni_hip_constraint_new(device, self.regex._h, off.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    data.ctypes.data_as(C.POINTER(C.c_uint8)) if data.size else None, len(self.tokens),
                                                    C.byref(self._h)))
        s, v, w = C.c_int32(), C.c_int32(), C.c_int32()
        check_error(lib().kjarni_hip_constraint_dims(self._h, C.byref(s), C.byref(v), C.byref(w)))
        self.states, self.vocab, self.words = int(s.value), int(v.value), int(w.value)

    def mask(self, state: int) -> np.ndarray:
        """The 64-bit words of one state's mask, from the device."""
        out = np.empty(self.words, np.uint64)
        check_error(lib().kjarni_hip_constraint_mask(self._h, state, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def counts(self) -> np.ndarray:
        out = np.empty(self.states, np.uint32)
        check_error(lib().kjarni_hip_constraint_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def close(self):
        if self._h:
            lib().kjarni_hip_constraint_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def result_dict(r: "_ffi.KjarniHipConstraintResult") -> Dict[str, int]:
    return {"final_state": int(r.final_state), "device_state": int(r.device_state), "accepted": int(r.accepted),
            "complete": int(r.complete), "violated": int(r.violated)}


# ---- grammars ----------------------------------------------------------------------------------------------------------------------

Rules = List[Tuple[str, str]]
_WS = "[ \\t\\n\\r]*"
_JSON_SCALAR = json_string() + "|" + number() + "|true|false|null"


def _value_rules(w: str) -> Rules:
    """value / object / array, with `w` (JSON's whitespace, or nothing) after { [ , : and after every value inside a container
    (so: before , } ]) and after a key; none around `value` itself, so that no call boundary sees it twice."""
    member = json_string() + w + ":" + w + "(?&value)" + w
    return [("value", "(?&object)|(?&array)|" + _JSON_SCALAR),
            ("object", "\\{" + w + "(?:" + member + "(?:," + w + member + ")*)?\\}"),
            ("array", "\\[" + w + "(?:(?&value)" + w + "(?:," + w + "(?&value)" + w + ")*)?\\]")]


def json_value(whitespace: bool = False) -> Rules:
    """Any JSON value, as rules for Grammar: value, object, array, rule 0 = value.  With whitespace=True, JSON's own [ \\t\\n\\r]*
    is allowed wherever JSON allows it; the whitespace around the top value needs a rule of its own in front, `json`, which is
    then rule 0 (a called rule cannot carry whitespace at its ends without a call boundary seeing it twice).  Nesting is bounded
    by GRAMMAR_MAX_DEPTH calls: a container inside a container costs two (value, then object or array), so 32 levels."""
    if not whitespace:
        return _value_rules("")
    return [("json", _WS + "(?&value)" + _WS)] + _value_rules(_WS)


_ANNOTATIONS = ("title", "description", "default", "examples", "$schema", "$defs", "$id", "$comment")


class _SchemaBuilder:
    def __init__(self, root: Any, whitespace: bool):
        self.root = root
        self.w = _WS if whitespace else ""
        self.defs: Dict[str, str] = {}       # $defs name -> rule name
        self.rules: Dict[str, Optional[str]] = {}
        self.order: List[str] = []
        self.any_value = False

    def build(self) -> Rules:
        self.rules["root"] = None
        self.order.append("root")
        self.rules["root"] = self.pattern(self.root)
        out: Rules = []
        if self.w:
            out.append(("json", self.w + "(?&root)" + self.w))
        out += [(n, self.rules[n]) for n in self.order]
        if self.any_value:
            out += _value_rules(self.w)
        return out

    def ref(self, target: str) -> str:
        if target == "#":
            return "(?&root)"
        if not target.startswith("#/$defs/"):
            raise ValueError("json_schema: unsupported $ref %r (only # and #/$defs/NAME)" % (target,))
        name = target[len("#/$defs/"):]
        defs = self.root.get("$defs", {}) if isinstance(self.root, dict) else {}
        if name not in defs:
            raise ValueError("json_schema: $ref to the undefined %r" % (target,))
        if name not in self.defs:
            rule = "def_%d" % len(self.defs)
            self.defs[name] = rule
            self.rules[rule] = None
            self.order.append(rule)
            self.rules[rule] = self.pattern(defs[name])
        return "(?&" + self.defs[name] + ")"

    def any(self) -> str:
        self.any_value = True
        return "(?&value)"

    @staticmethod
    def literal(v: Any) -> str:
        import json
        if v is not None and not isinstance(v, (bool, int, float, str)):
            raise ValueError("json_schema: enum / const take scalars only, got %r" % (v,))
        return escape(json.dumps(v, ensure_ascii=False))

    def pattern(self, s: Any) -> str:
        if s is True:
            return self.any()
        if not isinstance(s, dict):
            raise ValueError("json_schema: a schema is an object or true, got %r" % (s,))
        s = {k: v for k, v in s.items() if k not in _ANNOTATIONS}
        if not s:
            return self.any()
        known = {"$ref", "enum", "const", "anyOf", "oneOf", "type", "properties", "required", "additionalProperties", "items", "minItems",
                 "maxItems"}
        for k in s:
            if k not in known:
                raise ValueError("json_schema: unsupported keyword %r" % (k,))
        if "additionalProperties" in s and s["additionalProperties"] is not False:
            raise ValueError("json_schema: unsupported keyword 'additionalProperties' other than false")
        if "$ref" in s:
            return self.ref(s["$ref"])
        if "const" in s:
            return self.literal(s["const"])
        if "enum" in s:
            if not s["enum"]:
                raise ValueError("json_schema: an empty enum")
            return "(?:" + "|".join(self.literal(v) for v in s["enum"]) + ")"
        for key in ("anyOf", "oneOf"):
            if key in s:
                if not s[key]:
                    raise ValueError("json_schema: an empty " + key)
                return "(?:" + "|".join(self.pattern(x) for x in s[key]) + ")"
        t = s.get("type")
        if t is None:
            t = "object" if "properties" in s else "array" if "items" in s else None
            if t is None:
                raise ValueError("json_schema: a schema with neither type, enum, const, anyOf, oneOf nor $ref: %r" % (sorted(s),))
        if isinstance(t, list):
            if not t:
                raise ValueError("json_schema: an empty type list")
            return "(?:" + "|".join(self.typed(x, s) for x in t) + ")"
        return self.typed(t, s)

    def typed(self, t: str, s: Mapping[str, Any]) -> str:
        w = self.w
        if t == "string":
            return json_string()
        if t == "integer":
            return integer()
        if t == "number":
            return number()
        if t == "boolean":
            return "(?:true|false)"
        if t == "null":
            return "null"
        if t == "array":
            item = self.pattern(s["items"]) if "items" in s else self.any()
            lo, hi = int(s.get("minItems", 0)), s.get("maxItems")
            if lo < 0 or lo > 255 or (hi is not None and not 0 <= int(hi) <= 255):
                raise ValueError("json_schema: minItems / maxItems must be 0..255")
            if hi is not None and int(hi) < lo:
                raise ValueError("json_schema: maxItems below minItems")
            if hi is not None and int(hi) == 0:
                return "\\[" + w + "\\]"
            more = "(?:," + w + "(?:" + item + ")" + w + "){%d,%s}" % (max(lo - 1, 0), "" if hi is None else int(hi) - 1)
            body = "(?:" + item + ")" + w + more
            return "\\[" + w + (body if lo >= 1 else "(?:" + body + ")?") + "\\]"
        if t == "object":
            if "properties" not in s:
                if s.get("required"):
                    raise ValueError("json_schema: required names a property that is not declared")
                self.any_value = True
                return "(?&object)"
            props = s["properties"]
            required = list(s.get("required", []))
            for r in required:
                if r not in props:
                    raise ValueError("json_schema: required names the undeclared property %r" % (r,))
            fields = [("\"" + escape(_json_key(k)) + "\"" + w + ":" + w + "(?:" + self.pattern(v) + ")" + w, k in required) for k, v in props.items()]
            alts = []
            for i, (f, req) in enumerate(fields):   # f is the first property present: every earlier one is optional and left out
                alts.append(f + "".join("(?:," + w + g + ")" + ("" if greq else "?") for g, greq in fields[i + 1:]))
                if req:
                    break
            body = ""
            if alts:
                body = "(?:" + "|".join(alts) + ")" + ("" if any(req for _, req in fields) else "?")
            return "\\{" + w + body + "\\}"
        raise ValueError("json_schema: unsupported type %r" % (t,))


def json_schema(schema: Any, whitespace: bool = False) -> Rules:
    """The rules of the JSON values a schema admits.  Supported: type (object, array, string, integer, number, boolean, null, or
    a list of them), enum and const over scalars, properties in the declared order with required (an optional property may be
    left out; additionalProperties is taken as false; an object schema with no `properties` at all is any object), items with
    minItems / maxItems up to 255, anyOf / oneOf as alternation (a conflict between the alternatives is the compiler's refusal,
    passed on by Grammar), $ref to # and #/$defs/NAME (recursion becomes rule calls), {} and true for any value.  title,
    description, default, examples, $schema are ignored; any other keyword is a ValueError naming it.  Rule 0 is `root`, or with
    whitespace=True `json` (the whitespace around the top value)."""
    return _SchemaBuilder(schema, whitespace).build()


class Grammar:
    """Rules compiled to a stack automaton (no GPU).  action [states, 256] uint32 (bits 31..30: 0 none, 1 move, 2 call; next
    state in bits 11..0, a call's return state in bits 23..12), flags [states] (bit 0 accepting, bit 1 no_out), rule_of [states].
    A configuration is (state, stack) with the stack a tuple of return states, bottom first."""

    def __init__(self, rules: Sequence[Tuple[str, str]]):
        self.rules = [(str(n), str(p)) for n, p in rules]
        self._h = C.c_void_p()
        n = len(self.rules)
        names = (C.c_char_p * max(n, 1))(*[r[0].encode("utf-8") for r in self.rules])
        pats = (C.c_char_p * max(n, 1))(*[r[1].encode("utf-8") for r in self.rules])
        check_error(lib().kjarni_hip_grammar_compile(names, pats, n, C.byref(self._h)))
        s, k = C.c_int32(), C.c_int32()
        check_error(lib().kjarni_hip_grammar_dims(self._h, C.byref(s), C.byref(k)))
        self.states, self.kept_rules = int(s.value), int(k.value)
        self.action = np.empty((self.states, 256), np.uint32)
        self.flags = np.empty(self.states, np.uint8)
        self.rule_of = np.empty(self.states, np.uint16)
        check_error(lib().kjarni_hip_grammar_table(self._h, self.action.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   self.flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   self.rule_of.ctypes.data_as(C.POINTER(C.c_uint16))))

    start = (0, ())

    def walk(self, config: Tuple[int, Tuple[int, ...]], data: bytes, as_token: bool = False) -> Optional[Tuple[int, Tuple[int, ...]]]:
        """The configuration after `data` from `config`; None when the walk dies.  as_token: `data` is one token's bytes, and
        more than GRAMMAR_TOKEN_PUSHES of its own pushes held at once kill the walk (the rule the kernels keep)."""
        state, stack = config
        depth = len(stack)
        buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data.ljust(1, b"\0"))
        st = (C.c_uint16 * GRAMMAR_MAX_DEPTH)(*stack[:GRAMMAR_MAX_DEPTH])
        out = (C.c_uint16 * GRAMMAR_MAX_DEPTH)()
        q, d, alive = C.c_uint32(), C.c_int32(), C.c_int32()
        check_error(lib().kjarni_hip_grammar_walk(self._h, state, st, depth, buf, len(data), 1 if as_token else 0, C.byref(q), out, C.byref(d),
                                                  C.byref(alive)))
        if not alive.value:
            return None
        return int(q.value), tuple(int(out[i]) for i in range(d.value))

    def accepted(self, config) -> bool:
        return config is not None and all(self.flags[q] & 1 for q in (config[0],) + tuple(config[1]))

    def closed(self, config) -> bool:
        return config is not None and all(self.flags[q] & 2 for q in (config[0],) + tuple(config[1]))

    def matches(self, data: bytes) -> bool:
        return self.accepted(self.walk(self.start, data))

    def close(self):
        if self._h:
            lib().kjarni_hip_grammar_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GrammarConstraint:
    """Rules (or a compiled Grammar) and the vocabulary's token bytes, with the automaton and the token table on the device."""

    def __init__(self, rules, tokens: Sequence[bytes], device: int = 0):
        self.grammar = rules if isinstance(rules, Grammar) else Grammar(rules)
        self.tokens: List[bytes] = [bytes(t) for t in tokens]
        off, data = token_table(self.tokens)
        self._h = C.c_void_p()
        self.device = device
        check_error(lib().kjarni_hip_grammar_constraint_new(device, self.grammar._h, off.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                            data.ctypes.data_as(C.POINTER(C.c_uint8)) if data.size else None, len(self.tokens),
                                                            C.byref(self._h)))
        s, v = C.c_int32(), C.c_int32()
        check_error(lib().kjarni_hip_grammar_constraint_dims(self._h, C.byref(s), C.byref(v)))
        self.states, self.vocab = int(s.value), int(v.value)

    @staticmethod
    def _rows(configs, done):
        n = len(configs)
        states = np.array([c[0] for c in configs], np.uint32)
        depths = np.array([len(c[1]) for c in configs], np.int32)
        stacks = np.zeros((n, GRAMMAR_MAX_DEPTH), np.uint16)
        for r, c in enumerate(configs):
            if len(c) > 2:                      # (state, stack, all 64 stack words): what lies above the depth, for the tests
                stacks[r] = c[2]
            stacks[r, :min(len(c[1]), GRAMMAR_MAX_DEPTH)] = c[1][:GRAMMAR_MAX_DEPTH]   # (a deeper stack: the depth is refused natively)
        flags = np.zeros(n, np.int32) if done is None else np.ascontiguousarray(done, np.int32)
        return states, depths, stacks, flags

    def apply(self, logits: np.ndarray, configs, done=None, stop_ids: Sequence[int] = ()) -> np.ndarray:
        """grammar_apply_kernel alone: logits [rows, ld] float32, one configuration (state, stack) per row."""
        logits = np.ascontiguousarray(logits, np.float32)
        rows, ld = logits.shape
        states, depths, stacks, flags = self._rows(configs, done)
        stops = np.array(list(stop_ids), np.uint32)
        out = np.empty_like(logits)
        i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        check_error(lib().kjarni_hip_op_grammar_apply(self.device, self._h, logits.ctypes.data_as(C.POINTER(C.c_float)), rows, ld,
                                                      states.ctypes.data_as(u32), depths.ctypes.data_as(i32),
                                                      stacks.ctypes.data_as(C.POINTER(C.c_uint16)), flags.ctypes.data_as(i32),
                                                      stops.ctypes.data_as(u32) if stops.size else None, int(stops.size),
                                                      out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def advance(self, picked: Sequence[int], configs, done=None, stop_ids: Sequence[int] = (), log_count: int = 0, log_cap: int = 0):
        """grammar_advance_kernel alone.  Returns a dict: states, depths, stacks [rows, 64], done, violated, and with log_cap > 0
        state_log / depth_log [log_cap] (preset to 0xFFFFFFFF / -1)."""
        picks = np.array(list(picked), np.int32)
        states, depths, stacks, flags = self._rows(configs, done)
        flags = flags.copy()
        stops = np.array(list(stop_ids), np.uint32)
        violated = np.full(len(picks), -7, np.int32)
        slog = np.full(max(log_cap, 1), 0xFFFFFFFF, np.uint32)
        dlog = np.full(max(log_cap, 1), -1, np.int32)
        i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        check_error(lib().kjarni_hip_op_grammar_advance(self.device, self._h, picks.ctypes.data_as(i32), len(picks), states.ctypes.data_as(u32),
                                                        depths.ctypes.data_as(i32), stacks.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                        flags.ctypes.data_as(i32), stops.ctypes.data_as(u32) if stops.size else None,
                                                        int(stops.size), violated.ctypes.data_as(i32), log_count, log_cap,
                                                        slog.ctypes.data_as(u32) if log_cap > 0 else None,
                                                        dlog.ctypes.data_as(i32) if log_cap > 0 else None))
        return {"states": states, "depths": depths, "stacks": stacks, "done": flags, "violated": violated, "state_log": slog[:log_cap],
                "depth_log": dlog[:log_cap]}

    def close(self):
        if self._h:
            lib().kjarni_hip_grammar_constraint_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grammar_result_dict(r: "_ffi.KjarniHipGrammarResult") -> Dict[str, int]:
    return {"final_state": int(r.final_state), "device_state": int(r.device_state), "final_depth": int(r.final_depth),
            "device_depth": int(r.device_depth), "accepted": int(r.accepted), "complete": int(r.complete), "violated": int(r.violated)}


# ---- the lanes: an automaton per lane (the result struct, and the test hook of the two kernels) ----------------------------------------------------------------------------------------------

LANE_SLOTS = 64


def lane_result_dict(r: "_ffi.KjarniHipLaneAutomatonResult") -> Dict[str, int]:
    return {"kind": int(r.kind), "final_state": int(r.final_state), "device_state": int(r.device_state), "final_depth": int(r.final_depth),
            "device_depth": int(r.device_depth), "accepted": int(r.accepted), "complete": int(r.complete), "violated": int(r.violated)}


class LaneAutomata:
    """TEST HOOK, not part of the decoding interface (generate_wide_constrained and Generator.generate_batch are): the per-lane host
    arrays that kjarni_hip_op_lane_automaton_apply / _pick take, so that the two kernels can be run alone, as Constraint.apply and
    GrammarConstraint.apply / advance run theirs.  violated starts at -7 so that a caller can tell what a call wrote.  `lanes`: one entry per lane from lane 0, each None (kind 0), or a dict with
    "automaton" (a Constraint: a pattern lane, "state"; a GrammarConstraint: a grammar lane, "config" = (state, stack[, all 64
    stack words])), and optionally "done" and "stop_ids".  Lanes behind the list are kind 0."""

    def __init__(self, lanes):
        n = LANE_SLOTS
        self.kinds = np.zeros(n, np.int32)
        self.constraints = (C.c_void_p * n)()
        self.grammars = (C.c_void_p * n)()
        self.states = np.zeros(n, np.uint32)
        self.depths = np.zeros(n, np.int32)
        self.stacks = np.zeros((n, GRAMMAR_MAX_DEPTH), np.uint16)
        self.done = np.zeros(n, np.int32)
        self.stops = np.zeros((n, 16), np.uint32)
        self.n_stop = np.zeros(n, np.int32)
        self.violated = np.full(n, -7, np.int32)
        self._keep = list(lanes)
        for l, e in enumerate(lanes):
            if e is None:
                continue
            a = e["automaton"]
            stops = list(e.get("stop_ids", ()))
            self.n_stop[l] = len(stops)
            self.stops[l, :min(len(stops), 16)] = stops[:16]
            self.done[l] = 1 if e.get("done") else 0
            if isinstance(a, GrammarConstraint):
                self.kinds[l] = 2
                self.grammars[l] = a._h.value
                c = e.get("config", (0, []))
                self.states[l] = c[0]
                self.depths[l] = len(c[1])
                if len(c) > 2:
                    self.stacks[l] = c[2]
                self.stacks[l, :min(len(c[1]), GRAMMAR_MAX_DEPTH)] = c[1][:GRAMMAR_MAX_DEPTH]
            else:
                self.kinds[l] = 1
                self.constraints[l] = a._h.value
                self.states[l] = e.get("state", 0)

    def _args(self):
        i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        return (self.kinds.ctypes.data_as(i32), self.constraints, self.grammars, self.states.ctypes.data_as(u32), self.depths.ctypes.data_as(i32),
                self.stacks.ctypes.data_as(C.POINTER(C.c_uint16)), self.done.ctypes.data_as(i32), self.stops.ctypes.data_as(u32),
                self.n_stop.ctypes.data_as(i32))

    def apply(self, logits: np.ndarray, live, lanes: Optional[int] = None, first_lane: int = 0, vocab: Optional[int] = None,
              device: int = 0) -> np.ndarray:
        """lane_automaton_apply_kernel alone (kjarni_hip_op_lane_automaton_apply): logits [first_lane + lanes, ld] float32, live [64]."""
        logits = np.ascontiguousarray(logits, np.float32)
        rows, ld = logits.shape
        lanes = rows - first_lane if lanes is None else int(lanes)
        lv = np.zeros(LANE_SLOTS, np.int32)
        lv[:len(live)] = live
        out = np.empty_like(logits)
        check_error(lib().kjarni_hip_op_lane_automaton_apply(device, logits.ctypes.data_as(C.POINTER(C.c_float)), ld, ld if vocab is None else int(vocab),
                                                             lanes, int(first_lane), lv.ctypes.data_as(C.POINTER(C.c_int32)), *self._args(),
                                                             out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def pick(self, logits: np.ndarray, state, history: np.ndarray, capacity: int, lanes: Optional[int] = None, first_lane: int = 0,
             advance: int = 1, vocab: Optional[int] = None, device: int = 0):
        """The lanes' pick and the lane advance behind it (kjarni_hip_op_lane_automaton_pick): `state` is a _ffi.KjarniHipWideState
        (history [64, stride]) or a _ffi.KjarniHipLaneState (history [8, stride]), picked in place, as `history` (int32) and this
        object's states / depths / stacks / done; violated is written for the lanes of the range."""
        logits = np.ascontiguousarray(logits, np.float32)
        rows, ld = logits.shape
        lanes = rows - first_lane if lanes is None else int(lanes)
        wide = 1 if isinstance(state, _ffi.KjarniHipWideState) else 0
        if history.dtype != np.int32 or not history.flags["C_CONTIGUOUS"] or history.shape[0] != (64 if wide else 8):
            raise ValueError("history: a contiguous int32 array of 64 (wide state) or 8 rows")
        args = self._args()
        check_error(lib().kjarni_hip_op_lane_automaton_pick(device, wide, logits.ctypes.data_as(C.POINTER(C.c_float)), ld,
                                                            ld if vocab is None else int(vocab), lanes, int(first_lane),
                                                            C.cast(C.byref(state), C.c_void_p), history.ctypes.data_as(C.POINTER(C.c_int32)),
                                                            history.shape[1], int(capacity), int(advance), *args,
                                                            self.violated.ctypes.data_as(C.POINTER(C.c_int32))))
        return self
