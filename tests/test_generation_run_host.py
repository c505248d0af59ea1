"""The bookkeeping rule of the generation loops without a GPU: GenerationRun (kjarni_amd/csrc/generation_run.h) replayed on a
token stream through kjarni_generation_replay, against the rule written out below.

The rule: before a token is taken, the run must not be done, must have emitted fewer than max_new_tokens and must hold fewer
tokens than min(capacity, max_len or prompt + max_new_tokens); a stop id ends the run unemitted; any other token is pushed, the
callback is asked, then max_new_tokens is checked.  An emitted token is fed to another step unless the callback refused it or it
filled the context; the last token of max_new_tokens is fed by generate()'s processor / sampling loops (feed_last) and not by
the lanes.  With max_len = 0 that token also meets max_len = prompt + max_new_tokens, so the two agree: only an explicit larger
max_len tells them apart, which no C entry point of the decoders can set -- hence the assert lives here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kjarni_amd
from kjarni_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM = list(range(100, 108))


def rule(n_prompt, capacity, max_new, stream, max_len=0, stop_ids=(), default_stop_ids=(), cancel_after=-1, feed_last=False):
    stops = list(stop_ids) or list(default_stop_ids)
    limit = min(capacity, max_len or n_prompt + max_new)
    n, emitted, asked, fed, done = n_prompt, 0, 0, 0, False
    while not done and emitted < max_new and n < limit and asked < len(stream):
        tok, asked = stream[asked], asked + 1
        if tok in stops:
            break
        n, emitted = n + 1, emitted + 1
        cancelled = emitted == cancel_after
        done = cancelled or emitted >= max_new
        fed += int(not cancelled and n < limit and (feed_last or not done))
    return emitted, asked, fed


# (what, arguments, emitted, asked, fed with feed_last, fed without)
TABLE = [
    ("max_new_tokens = 0", dict(n_prompt=5, capacity=20, max_new=0), 0, 0, 0, 0),
    ("a prompt already at max_len", dict(n_prompt=5, capacity=20, max_new=4, max_len=5), 0, 0, 0, 0),
    ("a prompt already at the capacity", dict(n_prompt=20, capacity=20, max_new=4), 0, 0, 0, 0),
    ("a stop id as the first token", dict(n_prompt=5, capacity=20, max_new=4, stop_ids=[100]), 0, 1, 0, 0),
    ("a stop id as the last allowed token", dict(n_prompt=5, capacity=20, max_new=4, stop_ids=[103]), 3, 4, 3, 3),
    ("a stop id one past the limit (never asked)", dict(n_prompt=5, capacity=20, max_new=4, stop_ids=[104]), 4, 4, 3, 3),
    ("max_len binds before max_new_tokens", dict(n_prompt=5, capacity=20, max_new=8, max_len=8), 3, 3, 2, 2),
    ("the capacity binds before both", dict(n_prompt=5, capacity=7, max_new=8, max_len=12), 2, 2, 1, 1),
    ("the callback cancels at token 1", dict(n_prompt=5, capacity=20, max_new=4, cancel_after=1), 1, 1, 0, 0),
    ("the callback cancels at the last token", dict(n_prompt=5, capacity=20, max_new=4, cancel_after=4), 4, 4, 3, 3),
    ("an empty stop list falls back to the defaults", dict(n_prompt=5, capacity=20, max_new=4, default_stop_ids=[102]), 2, 3, 2, 2),
    ("an explicit stop list hides the defaults", dict(n_prompt=5, capacity=20, max_new=4, stop_ids=[103], default_stop_ids=[101]), 3, 4, 3, 3),
    ("a stream shorter than the run", dict(n_prompt=5, capacity=20, max_new=8, stream=STREAM[:3]), 3, 3, 3, 3),
    # the feed rule: generate()'s processor / sampling loops feed the last token of max_new_tokens, the lanes do not ...
    ("max_len past prompt + max_new_tokens", dict(n_prompt=5, capacity=20, max_new=4, max_len=20), 4, 4, 4, 3),
    # ... and with the default max_len that token fills the context, which nobody feeds
    ("the default max_len is met by the last token", dict(n_prompt=5, capacity=20, max_new=4), 4, 4, 3, 3),
]


@pytest.mark.parametrize("what,kw,emitted,asked,fed_last,fed_not", TABLE, ids=[t[0] for t in TABLE])
def test_table(what, kw, emitted, asked, fed_last, fed_not):
    kw = dict(kw)
    kw.setdefault("stream", STREAM)
    for feed_last, fed in ((True, fed_last), (False, fed_not)):
        got = kjarni_amd.generation_replay(feed_last=feed_last, **{("max_new_tokens" if k == "max_new" else k): v for k, v in kw.items()})
        n_emitted, n_asked, n_fed = got
        assert n_emitted == emitted and n_asked == asked, (what, got)
        assert n_fed == fed, (what, feed_last, got)
        assert got == rule(feed_last=feed_last, **kw), what


def test_the_processor_loops_feed_the_last_token_of_max_new_tokens_and_the_lanes_do_not():
    emitted, _, fed = kjarni_amd.generation_replay(6, 64, 5, STREAM, max_len=40, feed_last=True)
    assert emitted == 5 and fed == 5            # every emitted token runs a step: the cache ends at prompt + max_new_tokens
    emitted, _, fed = kjarni_amd.generation_replay(6, 64, 5, STREAM, max_len=40, feed_last=False)
    assert emitted == 5 and fed == 4            # the cache ends one row short


def test_random_cases_equal_the_rule():
    rng = np.random.default_rng(31)
    for _ in range(600):
        n_prompt, capacity = int(rng.integers(1, 12)), int(rng.integers(1, 24))
        capacity = max(capacity, n_prompt)
        kw = dict(n_prompt=n_prompt, capacity=capacity, max_new=int(rng.integers(0, 10)),
                  max_len=int(rng.choice([0, 0, int(rng.integers(1, 24))])),
                  stream=rng.integers(0, 6, int(rng.integers(0, 12))).tolist(),
                  stop_ids=rng.integers(0, 12, int(rng.integers(0, 3))).tolist(),
                  default_stop_ids=rng.integers(0, 12, int(rng.integers(0, 3))).tolist(),
                  cancel_after=int(rng.choice([-1, -1, int(rng.integers(1, 8))])), feed_last=bool(rng.integers(0, 2)))
        args = {("max_new_tokens" if k == "max_new" else k): v for k, v in kw.items()}
        assert kjarni_amd.generation_replay(**args) == rule(**kw), kw


def test_symbol_is_declared_bound_and_checks_its_pointers():
    L = kjarni_amd.lib()
    header = open(os.path.join(ROOT, "include", "kjarni_hip.h")).read()
    assert "kjarni_generation_replay(" in header and hasattr(L, "kjarni_generation_replay")
    restype, argtypes = _ffi.SIGNATURES["kjarni_generation_replay"]
    assert restype is C.c_int32 and len(argtypes) == 15
    assert callable(kjarni_amd.generation_replay)
    e, a = C.c_size_t(7), C.c_size_t(7)
    NULL_POINTER = L.kjarni_hip_prefix_keep(None, 0, None, 0, 0, None)
    assert NULL_POINTER != 0
    assert L.kjarni_generation_replay(1, 4, 2, 0, None, 0, None, 0, None, 0, -1, 0, None, C.byref(a), None) == NULL_POINTER
    assert L.kjarni_generation_replay(1, 4, 2, 0, None, 1, None, 0, None, 0, -1, 0, C.byref(e), C.byref(a), None) == NULL_POINTER
    assert L.kjarni_generation_replay(1, 4, 2, 0, None, 0, None, 0, None, 0, -1, 0, C.byref(e), C.byref(a), None) == 0  # n_fed may be NULL
    assert (e.value, a.value) == (0, 0)


def test_the_struct_alone_under_the_sanitizers(tmp_path):
    """generation_run.h is plain C++17: the stand-alone program runs this table under AddressSanitizer and UBSan (host code, its
    own main; nothing is loaded into this process)."""
    exe = str(tmp_path / "generation_run_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "kjarni_amd", "csrc"), os.path.join(ROOT, "tests", "generation_run_table.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(TABLE)} cases, 0 failed" in r.stdout
