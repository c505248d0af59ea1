"""Constrained decoding: patterns, the compiled DFA and the device constraint.

The string builders are pure Python and return patterns in the syntax the native compiler accepts (include/kjarni_hip.h:
kjarni_hip_regex_compile), with the meaning of Python's re.fullmatch(pattern, text, re.ASCII).  Only flat formats are built here:
nested or recursive JSON schemas are out of scope (a regular expression cannot count brackets).

    Regex        a compiled pattern: the byte DFA (host only, no GPU)
    Constraint   a Regex and a token table with their mask on the device: what HipDecoder.generate_constrained takes
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Mapping, Sequence, Tuple

import numpy as np

from . import _ffi
from ._ffi import check_error, lib

DEAD = 0xFFFF
MAX_STATES = 4096
MAX_STOPS = 16

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
