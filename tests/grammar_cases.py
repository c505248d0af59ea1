"""Grammar-constrained decoding restated in Python, shared by tests/test_grammar_host.py and tests/test_gpu_grammar.py: grammars
as small trees with their own recogniser (sets of end positions, no table involved), the walk of an exported action table with
the depth limit and the 16-push window of a token, the host automaton that tests/constraint_cases.py:oracle_run drives, and a
validator for the schema subset of kjarni_amd.constraints.json_schema.  Nothing here touches the GPU."""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_DEPTH = 64
TOKEN_PUSHES = 16
MAX_BYTE_STEPS = 64 + 256 + 2

# ---- grammars as trees ---------------------------------------------------------------------------------------------------------------

_META = set("\\.^$*+?{}[]()|\"")


class Node:
    def render(self) -> str:
        raise NotImplementedError


class Lit(Node):
    def __init__(self, text: str):
        self.data = text.encode()
        self.text = text

    def render(self):
        return "".join("\\" + c if c in _META else c for c in self.text)


class Cls(Node):
    """One byte out of `chars` (ASCII)."""

    def __init__(self, chars: str):
        self.chars = chars
        self.set = set(chars.encode())

    def render(self):
        return "[" + "".join("\\" + c if c in "\\]^-[" else c for c in self.chars) + "]"


class Seq(Node):
    def __init__(self, *kids: Node):
        self.kids = kids

    def render(self):
        return "".join(k.render() for k in self.kids)


class Alt(Node):
    def __init__(self, *kids: Node):
        self.kids = kids

    def render(self):
        return "(?:" + "|".join(k.render() for k in self.kids) + ")"


class Rep(Node):
    def __init__(self, kid: Node, lo: int = 0, hi: Optional[int] = None):
        self.kid, self.lo, self.hi = kid, lo, hi

    def render(self):
        q = {(0, None): "*", (1, None): "+", (0, 1): "?"}.get((self.lo, self.hi))
        if q is None:
            q = "{%d,%s}" % (self.lo, "" if self.hi is None else self.hi)
        return "(?:" + self.kid.render() + ")" + q


class Call(Node):
    def __init__(self, name: str):
        self.name = name

    def render(self):
        return "(?&" + self.name + ")"


def rules_of(grammar: Sequence[Tuple[str, Node]]) -> List[Tuple[str, str]]:
    return [(n, t.render()) for n, t in grammar]


def ends(grammar: Dict[str, Node], node: Node, data: bytes, i: int, memo: Optional[dict] = None, depth: int = 0,
         max_depth: Optional[int] = None) -> frozenset:
    """The positions where a string of `node` starting at data[i] can end.  Memoised per (node, position, call depth); the
    grammars of the tests are not left recursive, so a call at the same position never meets itself.  max_depth: calls open at
    once beyond which nothing matches (the automaton's limit is part of the language)."""
    memo = {} if memo is None else memo
    key = (id(node), i, depth if max_depth is not None else 0)
    if key in memo:
        return memo[key]
    if isinstance(node, Lit):
        out = frozenset([i + len(node.data)]) if data[i:i + len(node.data)] == node.data else frozenset()
    elif isinstance(node, Cls):
        out = frozenset([i + 1]) if i < len(data) and data[i] in node.set else frozenset()
    elif isinstance(node, Seq):
        cur = {i}
        for k in node.kids:
            cur = set().union(*[ends(grammar, k, data, j, memo, depth, max_depth) for j in cur]) if cur else set()
        out = frozenset(cur)
    elif isinstance(node, Alt):
        out = frozenset().union(*[ends(grammar, k, data, i, memo, depth, max_depth) for k in node.kids])
    elif isinstance(node, Rep):
        cur, result, n = {i}, set(), 0
        if node.lo == 0:
            result.add(i)
        while cur and (node.hi is None or n < node.hi):
            nxt = set()
            for j in cur:
                nxt |= ends(grammar, node.kid, data, j, memo, depth, max_depth)
            n += 1
            if n >= node.lo:
                new = nxt - result
                result |= nxt
                if not new and node.hi is None:   # every position here was taken one step further at an earlier count >= lo
                    break
            cur = nxt
        out = frozenset(result)
    elif isinstance(node, Call):
        if max_depth is not None and depth >= max_depth:
            out = frozenset()
        else:
            out = ends(grammar, grammar[node.name], data, i, memo, depth + 1, max_depth)
    else:
        raise TypeError(node)
    memo[key] = out
    return out


def matches(grammar: Sequence[Tuple[str, Node]], data: bytes, max_depth: Optional[int] = None) -> bool:
    g = dict(grammar)
    return len(data) in ends(g, grammar[0][1], data, 0, {}, 0, max_depth)


_D = Cls("0123456789")
BRACKETS = [("s", Rep(Alt(Seq(Lit("("), Rep(Call("s"), 0, 1), Lit(")")), Seq(Lit("["), Rep(Call("s"), 0, 1), Lit("]"))), 1))]
ANBN = [("s", Seq(Lit("a"), Rep(Call("s"), 0, 1), Lit("b")))]
LISTS = [("v", Alt(Rep(_D, 1), Seq(Lit("["), Rep(Seq(Call("v"), Rep(Seq(Lit(","), Call("v")))), 0, 1), Lit("]"))))]
CHAIN = [("a", Seq(Call("b"), Lit("w"))), ("b", Seq(Call("c"), Lit("v"))), ("c", Seq(Call("d"), Lit("u"))), ("d", Rep(Cls("xy"), 1))]
FLAT = [("s", Alt(Seq(Lit("a"), Rep(Alt(Lit("b"), Lit("c"))), Lit("d")), Rep(_D, 1, 3)))]
# name -> (grammar, alphabet, longest string enumerated)
TREES = {"brackets": (BRACKETS, "()[]", 8), "anbn": (ANBN, "ab", 12), "lists": (LISTS, "[],01", 7), "chain": (CHAIN, "xywvu", 6),
         "flat": (FLAT, "abcd01", 5)}


# ---- the table walk ------------------------------------------------------------------------------------------------------------------

Config = Tuple[int, Tuple[int, ...]]
START: Config = (0, ())


def walk(action: np.ndarray, flags: np.ndarray, config: Optional[Config], data: bytes, as_token: bool = False) -> Optional[Config]:
    """The configuration after `data`, None when the walk dies: the loop of kjarni_hip.h restated, with the depth limit and, for
    a token, the window of 16 own pushes."""
    if config is None:
        return None
    q, stack = config[0], list(config[1])
    own = 0
    for b in data:
        for step in range(MAX_BYTE_STEPS + 1):
            if step >= MAX_BYTE_STEPS:
                return None
            a = int(action[q, b])
            kind = a >> 30
            if kind == 1:
                q = a & 0xFFF
                break
            if kind == 2:
                if len(stack) >= MAX_DEPTH or (as_token and own >= TOKEN_PUSHES):
                    return None
                stack.append((a >> 12) & 0xFFF)
                own += 1
                q = a & 0xFFF
                continue
            if not (flags[q] & 1) or not stack:
                return None
            q = stack.pop()
            own = max(own - 1, 0)
    return q, tuple(stack)


def accepted(flags: np.ndarray, config: Optional[Config]) -> bool:
    return config is not None and all(flags[q] & 1 for q in (config[0],) + config[1])


def closed(flags: np.ndarray, config: Optional[Config]) -> bool:
    return config is not None and all(flags[q] & 2 for q in (config[0],) + config[1])


def own_pushes_peak(action: np.ndarray, flags: np.ndarray, config: Config, data: bytes) -> int:
    """The most own pushes the walk of `data` holds at once (no window applied); -1 when it dies for another reason."""
    q, stack = config[0], list(config[1])
    own = peak = 0
    for b in data:
        while True:
            a = int(action[q, b])
            kind = a >> 30
            if kind == 1:
                q = a & 0xFFF
                break
            if kind == 2:
                if len(stack) >= MAX_DEPTH:
                    return -1
                stack.append((a >> 12) & 0xFFF)
                own += 1
                peak = max(peak, own)
                q = a & 0xFFF
                continue
            if not (flags[q] & 1) or not stack:
                return -1
            q = stack.pop()
            own = max(own - 1, 0)
    return peak


def apply_reference(action, flags, tokens: Sequence[bytes], logits: np.ndarray, configs, done, stops) -> np.ndarray:
    """What grammar_apply_kernel must leave: a copy of `logits` with -inf where the walker masks (bits kept elsewhere)."""
    out = logits.copy()
    V = len(tokens)
    for r, c in enumerate(configs):
        if done[r]:
            continue
        cfg = (c[0], tuple(c[1]))
        for t in range(V):
            if t in stops:
                ok = accepted(flags, cfg)
            else:
                ok = len(tokens[t]) > 0 and walk(action, flags, cfg, tokens[t], True) is not None
            if not ok:
                out[r, t] = -np.inf
    return out


class _ByConfig:
    def __init__(self, fn):
        self.fn = fn

    def __getitem__(self, config):
        return self.fn(config)


class HostGrammar:
    """The exported table, the token bytes and a call's stop ids, with the attributes constraint_cases.oracle_run reads: start,
    legal(q), step(q, tok), stops, and closed[q] / accepting[q] indexable by configuration."""

    def __init__(self, grammar, tokens: Sequence[bytes], stops: Sequence[int]):
        self.action, self.flags = grammar.action, grammar.flags
        self.tokens, self.stops = list(tokens), list(stops)
        self.start = START
        self.accepting = _ByConfig(lambda c: accepted(self.flags, c))
        self.closed = _ByConfig(lambda c: closed(self.flags, c))
        self._legal: Dict[Config, np.ndarray] = {}
        self._first = np.array([t[0] if t else -1 for t in self.tokens])

    def legal(self, config: Config) -> np.ndarray:
        if config not in self._legal:
            ok = np.zeros(len(self.tokens), bool)
            for t, data in enumerate(self.tokens):
                ok[t] = len(data) > 0 and walk(self.action, self.flags, config, data, True) is not None
            for s in self.stops:
                if 0 <= s < ok.size:
                    ok[s] = accepted(self.flags, config)
            self._legal[config] = ok
        return self._legal[config]

    def step(self, config: Config, tok: int):
        nxt = walk(self.action, self.flags, config, self.tokens[tok], True) if self.tokens[tok] else None
        return 0xFFFF if nxt is None else nxt       # (oracle_run compares with DEAD)

    def text(self, ids: Sequence[int]) -> bytes:
        return b"".join(self.tokens[i] for i in ids)

    def config_after(self, ids: Sequence[int]) -> Optional[Config]:
        c = self.start
        for i in ids:
            c = walk(self.action, self.flags, c, self.tokens[i], True)
            if c is None:
                return None
        return c


BRACKET_WORDS = ["[", "]", "[]", "[[", "]]", "],", ",[", "[1", "1]", "{", "}", "}}", "{}", "\"}]", "{\"a\":[", "\"a\":", "[[[", "]]]", "null", "true",
                 "false", "1,", ",\"", "\"", "\"a\"", ":", ",", "a", "e", "0", "1", "2", "-", ".", " ", "é", "\xc3".encode("latin1"), "\xa9".encode("latin1"),
                 "u", "l", "r", "t", "f", "ul"]     # (with the base table's single letters, every prefix of null / true / false can go on)


def model_tokens(vocab: int, specials: Sequence[int] = (0, 1, 2, 3), seed: int = 0) -> List[bytes]:
    """constraint_cases.model_tokens extended by bracket tokens: the special ids have no bytes, then the bracket words above
    (tokens that push, pop, and do both inside themselves), then the base table's tokens."""
    from tests import constraint_cases as CC
    base = [t for t in CC.model_tokens(vocab, specials=(), seed=seed) if t]
    pool = [w if isinstance(w, bytes) else w.encode() for w in BRACKET_WORDS] + base
    out: List[bytes] = []
    for i in range(vocab):
        out.append(b"" if i in specials else pool.pop(0))
    return out


# ---- JSON: documents and the schema subset -------------------------------------------------------------------------------------------

def no_space_outside_strings(text: str) -> bool:
    """For a text json.loads accepts: no whitespace outside its strings (what whitespace=False admits)."""
    inside = False
    i = 0
    while i < len(text):
        c = text[i]
        if inside:
            if c == "\\":
                i += 1
            elif c == "\"":
                inside = False
        elif c == "\"":
            inside = True
        elif c in " \t\n\r":
            return False
        i += 1
    return True


class Obj(list):
    """A JSON object as its (key, value) pairs in the order of the text, duplicates kept."""


def _no_constant(name):
    raise ValueError("not JSON: " + name)


def parse(data: bytes):
    """(ok, value, text): strict JSON from UTF-8 bytes (no NaN / Infinity, no BOM, no other encoding guessed)."""
    try:
        text = data.decode("utf-8")
        return True, json.loads(text, object_pairs_hook=Obj, parse_constant=_no_constant), text
    except (ValueError, RecursionError):
        return False, None, None


def random_document(rng, depth: int = 0):
    kind = int(rng.integers(0, 9 if depth < 4 else 6))
    if kind == 0:
        return None
    if kind == 1:
        return bool(rng.integers(0, 2))
    if kind == 2:
        return int(rng.integers(-1000, 1000))
    if kind == 3:
        return float(np.round(rng.standard_normal() * 10 ** int(rng.integers(-3, 6)), 4))
    if kind in (4, 5):
        alphabet = ["a", "b", " ", "\"", "\\", "\n", "é", "€", "😀", "\t", "/", "{", "]", "\x7f"]
        return "".join(alphabet[int(j)] for j in rng.integers(0, len(alphabet), int(rng.integers(0, 6))))
    if kind in (6, 7):
        return [random_document(rng, depth + 1) for _ in range(int(rng.integers(0, 4)))]
    return {"k%d" % j + ("é" if rng.integers(0, 4) == 0 else ""): random_document(rng, depth + 1) for j in range(int(rng.integers(0, 4)))}


_IGNORED = ("title", "description", "default", "examples", "$schema", "$defs")


def valid(schema, value, root=None) -> bool:
    """Does a parsed value (objects as Obj) satisfy the schema, under the subset json_schema builds: declared property order,
    no additional properties, integer = an int in the text."""
    root = schema if root is None else root
    if schema is True:
        return True
    s = {k: v for k, v in schema.items() if k not in _IGNORED}
    if not s:
        return True
    if "$ref" in s:
        ref = s["$ref"]
        return valid(root if ref == "#" else root["$defs"][ref[len("#/$defs/"):]], value, root)
    if "const" in s:
        return type(value) is type(s["const"]) and value == s["const"]
    if "enum" in s:
        return any(type(value) is type(v) and value == v for v in s["enum"])
    for key in ("anyOf", "oneOf"):
        if key in s:
            return any(valid(x, value, root) for x in s[key])
    t = s.get("type")
    if t is None:
        t = "object" if "properties" in s else "array"
    if isinstance(t, list):
        return any(valid(dict(s, type=x), value, root) for x in t)
    if t == "string":
        return isinstance(value, str)
    if t == "integer":
        return isinstance(value, int) and not isinstance(value, bool)
    if t == "number":
        return isinstance(value, (int, float)) and not isinstance(value, bool)
    if t == "boolean":
        return isinstance(value, bool)
    if t == "null":
        return value is None
    if t == "array":
        if isinstance(value, Obj) or not isinstance(value, list):
            return False
        if len(value) < s.get("minItems", 0) or ("maxItems" in s and len(value) > s["maxItems"]):
            return False
        return all(valid(s.get("items", True), v, root) for v in value)
    if t == "object":
        if not isinstance(value, Obj):
            return False
        if "properties" not in s:
            return True
        names = list(s["properties"])
        required = set(s.get("required", []))
        at = 0
        for k, v in value:
            while at < len(names) and names[at] != k:
                if names[at] in required:
                    return False
                at += 1
            if at == len(names) or not valid(s["properties"][k], v, root):
                return False
            at += 1
        return not any(n in required for n in names[at:])
    raise ValueError(t)


def random_instance(schema, rng, root=None, depth: int = 0):
    """A value the schema admits (plain dicts, declared order)."""
    root = schema if root is None else root
    if schema is True or not {k: v for k, v in schema.items() if k not in _IGNORED}:
        return random_document(rng, 3)
    s = schema
    if "$ref" in s:
        ref = s["$ref"]
        return random_instance(root if ref == "#" else root["$defs"][ref[len("#/$defs/"):]], rng, root, depth + 1)
    if "const" in s:
        return s["const"]
    if "enum" in s:
        return s["enum"][int(rng.integers(0, len(s["enum"])))]
    for key in ("anyOf", "oneOf"):
        if key in s:
            return random_instance(s[key][int(rng.integers(0, len(s[key])))], rng, root, depth)
    t = s.get("type") or ("object" if "properties" in s else "array")
    if isinstance(t, list):
        t = t[int(rng.integers(0, len(t)))]
    if t == "string":
        return "".join(["a", "é", "\"", " ", "\\"][int(j)] for j in rng.integers(0, 5, int(rng.integers(0, 5))))
    if t == "integer":
        return int(rng.integers(-50, 50))
    if t == "number":
        return float(np.round(rng.standard_normal() * 100, 3))
    if t == "boolean":
        return bool(rng.integers(0, 2))
    if t == "null":
        return None
    if t == "array":
        lo = s.get("minItems", 0)
        hi = s.get("maxItems", lo + 3)
        n = int(rng.integers(lo, hi + 1)) if depth < 4 else lo
        return [random_instance(s.get("items", True), rng, root, depth + 1) for _ in range(n)]
    if t == "object":
        if "properties" not in s:
            return {"x": 1}
        required = set(s.get("required", []))
        return {k: random_instance(v, rng, root, depth + 1) for k, v in s["properties"].items()
                if k in required or (depth < 4 and rng.integers(0, 2))}
    raise ValueError(t)
