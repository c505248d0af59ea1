"""Constrained decoding in the lanes on the GPU: the lane apply kernel alone against constraint_cases.allowed_matrix and
grammar_cases' table walker, the pick + lane advance alone on both state layouts with every branch in neighbouring lanes, then
kjarni_hip_decoder_generate_wide_constrained over the 72 prompts of tests/lane_constraint_cases.py at every width against the
single-stream loops and the float64 references, the loops it works together with (processors, records, callbacks, prefix reuse,
GGUF at 8 lanes, the MoE fixture), the refusals by prompt index, and Generator.generate_batch under a pattern and a grammar."""
import json
import re

import numpy as np
import pytest

from tests import constraint_cases as CC
from tests import gpt2_fixture as G
from tests import grammar_cases as GC
from tests import lane_constraint_cases as LCC
from tests import lanes_cases as LC
from tests import token_select_cases as TS
from tests import wide_cases as WC

pytestmark = pytest.mark.gpu
CTX = LCC.LANE_CONTEXT


def _K():
    from kjarni_amd import constraints
    return constraints


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the lane apply alone -----------------------------------------------------------------------------------------------------------

class _Automata:
    """Two patterns and a bracket grammar over one token table of V tokens, on the device and on the host."""

    def __init__(self, V):
        K = _K()
        self.V = V
        self.tokens = GC.model_tokens(V)
        if V > 1000:                                   # a production vocabulary: the table's words, then seeded bracket / digit strings
            rng = np.random.default_rng(V)
            alphabet = np.frombuffer(b"()[]0123456789-yesno", np.uint8)
            for i in range(400, V):
                self.tokens[i] = alphabet[rng.integers(0, alphabet.size, int(rng.integers(1, 6)))].tobytes()
            self.tokens[V - 1] = b"()"
        self.pa = K.Constraint(K.choices(LCC.CHOICES), self.tokens)
        self.pb = K.Constraint(K.integer(), self.tokens)
        self.g = K.GrammarConstraint(GC.rules_of(GC.BRACKETS), self.tokens)
        self.allowed = {id(self.pa): CC.allowed_matrix(self.pa.regex.trans, self.tokens),
                        id(self.pb): CC.allowed_matrix(self.pb.regex.trans, self.tokens)}
        self.action, self.flags = self.g.grammar.action, self.g.grammar.flags
        self._legal = {}

    def config(self, opens):
        c = GC.walk(self.action, self.flags, GC.START, b"[" * opens)   # (the table's bracket words are square)
        assert c is not None
        return c

    def grammar_legal(self, cfg, stops):
        key = (cfg, tuple(stops))
        if key not in self._legal:
            row = np.zeros((1, self.V), np.float32)
            self._legal[key] = np.isfinite(GC.apply_reference(self.action, self.flags, self.tokens, row, [cfg], [0], list(stops))[0])
        return self._legal[key]


_AUT = {}


def _automata(V):
    if V not in _AUT:
        _AUT[V] = _Automata(V)
    return _AUT[V]


def _mix(A, lanes):
    """lane -> (spec for LaneAutomata, live, the tokens that must keep their bits (None: the whole row)).  Cycled: pattern A at its
    start with stop ids (not accepting), the grammar at depth 0, kind 0, pattern B in an accepting state with stop ids, the grammar at
    depth 1, a frozen lane, a done row, the grammar at depths 63 and 64.  Past nine lanes the last lane is pattern B accepting with
    stop ids (among nine, lane 3 is)."""
    stops = [5, 10, A.V - 1]
    qb = CC.walk(A.pb.regex.trans, A.pb.regex.start, b"12")
    assert A.pb.regex.accepting[qb] and not A.pb.regex.closed[qb] and not A.pa.regex.accepting[A.pa.regex.start]
    c1, c63, c64 = A.config(2), A.config(64), A.config(65)
    assert (len(c1[1]), len(c63[1]), len(c64[1])) == (1, 63, 64)

    def pattern(con, q, done=0, st=stops):
        legal = A.allowed[id(con)][q].copy()
        for s in st:
            legal[s] = bool(con.regex.accepting[q])
        return dict(automaton=con, state=q, done=done, stop_ids=st), legal

    def grammar(cfg, st=()):
        return dict(automaton=A.g, config=cfg, stop_ids=list(st)), A.grammar_legal(cfg, st)

    kinds = [lambda: pattern(A.pa, A.pa.regex.start) + (1,), lambda: grammar(GC.START) + (1,), lambda: (None, None, 1),
             lambda: pattern(A.pb, qb) + (1,), lambda: grammar(c1, stops) + (1,), lambda: (pattern(A.pa, A.pa.regex.start)[0], None, 0),
             lambda: (pattern(A.pb, qb, done=1)[0], None, 1), lambda: grammar(c63) + (1,), lambda: grammar(c64) + (1,)]
    out = [kinds[l % len(kinds)]() for l in range(lanes)]
    if lanes > 9:
        out[-1] = pattern(A.pb, qb) + (1,)
    return out


def _apply_mix(A, mix, ld, seed=0, rows=None):
    K = _K()
    lanes = len(mix)
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((rows or lanes, ld)).astype(np.float32)
    logits[:, A.V:] = np.nan                            # canaries behind every row
    logits[0, 7] = np.float32(-0.0)
    la = K.LaneAutomata([m[0] for m in mix])
    before = [x.copy() for x in (la.states, la.depths, la.stacks, la.done)]
    out = la.apply(logits, [m[2] for m in mix], lanes=lanes, vocab=A.V)
    assert all((a == b).all() for a, b in zip(before, (la.states, la.depths, la.stacks, la.done)))
    return logits, out


def _check_apply(A, mix, logits, out):
    for l, (spec, legal, live) in enumerate(mix):
        tail = slice(A.V, None)
        assert (_bits(out[l, tail]) == _bits(logits[l, tail])).all(), f"lane {l}: wrote behind the vocabulary"
        if legal is None:                                # kind 0, frozen, done: the row is left alone
            assert (_bits(out[l]) == _bits(logits[l])).all(), f"lane {l}: an untouched lane was written"
            continue
        assert (_bits(out[l, :A.V][legal]) == _bits(logits[l, :A.V][legal])).all(), f"lane {l}: an allowed logit was rewritten"
        assert np.isneginf(out[l, :A.V][~legal]).all(), f"lane {l}: a masked logit survived"


@pytest.mark.parametrize("V", [257, 320])
@pytest.mark.parametrize("lanes", [1, 9, 64])
def test_lane_apply_alone_against_the_host_walks(lanes, V):
    A = _automata(V)
    mix = _mix(A, lanes)
    logits, out = _apply_mix(A, mix, V + 7)
    _check_apply(A, mix, logits, out)
    again = _apply_mix(A, mix, V + 7)[1]
    assert (_bits(again) == _bits(out)).all(), "the same call twice gives other bits"
    if lanes == 9:                                       # the same nine lanes inside a launch of 64
        wide = _mix(A, 64)
        wide[:9] = mix
        l64, o64 = _apply_mix(A, wide, V + 7)
        assert (_bits(l64[:9]) == _bits(logits)).all() and (_bits(o64[:9]) == _bits(out)).all()
    if lanes >= 9:
        # stop ids in the first lane (not accepting: masked) and in the last (accepting: kept), whatever their bytes
        acc = 3 if lanes == 9 else lanes - 1
        assert np.isneginf(out[0, [5, 10, V - 1]]).all() and np.isfinite(out[acc, [5, 10, V - 1]]).all()
        assert np.isneginf(out[8, A.tokens.index(b"[")]) and np.isfinite(out[7, A.tokens.index(b"[")])   # depth 64 refuses a push, 63 takes it
        # a sub-range: lanes [3, 6) alone; the rows in front of it and behind it keep every bit
        K = _K()
        la = K.LaneAutomata([m[0] for m in mix])
        part = la.apply(logits[:6], [m[2] for m in mix], lanes=3, first_lane=3, vocab=V)
        assert (_bits(part[:3]) == _bits(logits[:3])).all() and (_bits(part[3:6]) == _bits(out[3:6])).all()


def test_lane_apply_at_a_production_vocabulary():
    V = 151936
    A = _automata(V)
    mix = _mix(A, 9)
    logits, out = _apply_mix(A, mix, V + 3)
    _check_apply(A, mix, logits, out)
    assert np.isfinite(out[1, V - 1]) and np.isneginf(out[8, V - 1]) and np.isfinite(out[7, V - 1])   # "()" at depths 0, 64, 63


# ---- pick + advance alone -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wide", [1, 0])
def test_pick_and_advance_every_branch(wide):
    from kjarni_amd import _ffi
    K = _K()
    V = 320
    A = _automata(V)
    tok = A.tokens.index
    rows, stride, cap, UNT = (64 if wide else 8), 6, 40, -77
    hc = CC.HostConstraint(A.pa.regex, A.tokens, [2, 3])
    q0 = hc.start
    q1 = hc.step(q0, tok(b"1"))                          # "1": not accepting, "12" and "100" go on
    q10 = hc.step(q1, tok(b"0"))
    q_yes = hc.step(q0, tok(b"yes"))
    qi = CC.walk(A.pb.regex.trans, A.pb.regex.start, b"12")
    assert hc.closed[q_yes] and not hc.accepting[q1] and hc.step(q1, tok(b"2")) == q_yes
    c1, c63, c64 = A.config(2), A.config(64), A.config(65)
    sentinel = np.full(64, 0x0ABC, np.uint16)
    # lane: (spec, pick, state changes, expected (state / config, done, violated, live))
    plan = [
        (dict(automaton=A.pb, state=qi, stop_ids=[2, 3]), 2, {}, (qi, 1, 0, 0)),                       # stop id, accepting: done, dead
        (dict(automaton=A.pa, state=q0, stop_ids=[2, 3]), 3, {}, (q0, 1, 1, 0)),                       # stop id, not accepting: violated
        (dict(automaton=A.pa, state=q1, stop_ids=[2, 3]), tok(b"2"), {}, (q_yes, 1, 0, 0)),            # closed: done, live cleared
        (dict(automaton=A.pa, state=q0, stop_ids=[2, 3]), tok(b"]"), {}, (q0, 1, 1, 0)),               # dead walk
        (dict(automaton=A.pa, state=q0, stop_ids=[2, 3]), tok(b"1"), {"limit": True}, (q1, 0, 0, 0)),  # the limit: walked, the pick's rule ends it
        (dict(automaton=A.pa, state=q1, stop_ids=[2, 3]), tok(b"0"), {"full": True}, (q10, 0, 0, 0)),  # a full cache
        (dict(automaton=A.pa, state=q0, stop_ids=[2, 3]), 0, {}, (q0, 1, 1, 0)),                       # a token of no bytes
        (dict(automaton=A.g, config=(c63[0], c63[1], sentinel)), tok(b"["), {}, (GC.walk(A.action, A.flags, c63, b"["), 0, 0, 1)),
    ]
    plan += [
        (dict(automaton=A.g, config=(c64[0], c64[1], sentinel)), tok(b"["), {}, (c64, 1, 1, 0)),    # the 65th push is refused
        (dict(automaton=A.g, config=(c1[0], c1[1], sentinel)), tok(b"]]"), {}, (GC.walk(A.action, A.flags, c1, b"]]"), 0, 0, 1)),
        (None, 17, {}, None),                                                                       # kind 0: the plain pick
        (dict(automaton=A.pa, state=q0, stop_ids=[2, 3]), tok(b"1"), {"frozen": True}, (q0, 0, -7, 0)),
        (dict(automaton=A.pa, state=q0, done=1, stop_ids=[2, 3]), tok(b"]"), {}, (q0, 1, 0, 1)),    # a done row no longer moves
        (dict(automaton=A.g, config=(0, (), sentinel), stop_ids=[2]), tok(b"[]"), {}, (GC.walk(A.action, A.flags, GC.START, b"[]"), 0, 0, 1)),
    ]
    assert GC.walk(A.action, A.flags, c64, b"[") is None and len(plan[7][3][0][1]) == 64

    def launch(plan):                                    # one launch over the lanes of `plan`, every branch checked
        n = len(plan)
        logits = np.random.default_rng(wide).standard_normal((n, V)).astype(np.float32)
        st = _ffi.KjarniHipWideState() if wide else _ffi.KjarniHipLaneState()
        hist = np.full((rows, stride), UNT, np.int32)
        for l, (spec, pick, how, _) in enumerate(plan):
            logits[l, pick] = 9.0
            assert TS.last_max(logits[l]) == pick
            st.token[l], st.pos[l], st.count[l], st.limit[l], st.live[l] = UNT - l, 10 + l, l % 3, 1 << 20, 0 if how.get("frozen") else 1
            if how.get("limit"):
                st.limit[l] = st.count[l] + 1
            if how.get("full"):
                st.pos[l] = cap - 1
            st.n_stop[l] = 2                                  # the lane's own stop rule holds the same ids
            st.stop[l][0], st.stop[l][1] = 2, 3
        before = {f: [getattr(st, f)[l] for l in range(rows)] for f in ("token", "pos", "live", "count")}
        la = K.LaneAutomata([p[0] for p in plan])
        la.pick(logits, st, hist, cap, lanes=n, advance=1)
        for l, (spec, pick, how, want) in enumerate(plan):
            cnt = before["count"][l]
            if how.get("frozen"):
                assert (hist[l] == UNT).all() and [getattr(st, f)[l] for f in before] == [before[f][l] for f in before]
                assert la.states[l] == want[0] and la.done[l] == 0
                continue
            # the pick's own rule (token_select_cases.last_max; count, pos, history)
            assert hist[l, cnt] == pick and (np.delete(hist[l], cnt) == UNT).all(), f"lane {l}"
            assert st.count[l] == cnt + 1 and st.pos[l] == before["pos"][l] + 1, f"lane {l}"
            if want is None:
                assert st.live[l] == 1 and st.token[l] == pick
                continue
            state, done, bad, live = want
            assert (la.done[l], la.violated[l], st.live[l]) == (done, bad, live), f"lane {l}: {(la.done[l], la.violated[l], st.live[l])}"
            if isinstance(state, tuple):                      # a configuration: state, depth, the stack up to the depth, the sentinel above
                top = max(len(state[1]), len(spec["config"][1]))
                assert la.states[l] == state[0] and la.depths[l] == len(state[1]) and tuple(la.stacks[l, :len(state[1])]) == tuple(state[1]), f"lane {l}"
                assert (la.stacks[l, top:] == 0x0ABC).all(), f"lane {l}: stack words above the depth were written"
            else:
                assert la.states[l] == state, f"lane {l}"
            if live:
                assert st.token[l] == pick                    # the token hand-over
        assert (hist[n:] == UNT).all()

    # the 8-lane layout takes the fourteen branches in two launches
    for part in ([plan] if wide else [plan[:8], plan[8:]]):
        launch(part)
    n = 8
    # a sub-range with first_lane > 0: the lanes in front of it and behind it keep everything
    logits = np.random.default_rng(7).standard_normal((5, V)).astype(np.float32)
    for l in range(5):
        logits[l, plan[l][1]] = 9.0
    st2 = _ffi.KjarniHipWideState() if wide else _ffi.KjarniHipLaneState()
    for l in range(n):
        st2.live[l], st2.limit[l], st2.count[l] = 1, 1 << 20, 1
    hist2 = np.full((rows, stride), UNT, np.int32)
    la2 = K.LaneAutomata([p[0] for p in plan])
    la2.pick(logits[:5], st2, hist2, cap, lanes=3, first_lane=2, advance=0)
    assert (hist2[:2] == UNT).all() and (hist2[5:] == UNT).all() and [st2.count[l] for l in range(6)] == [1, 1, 2, 2, 2, 1]
    assert [hist2[l, 1] for l in (2, 3, 4)] == [plan[l][1] for l in (2, 3, 4)] and st2.pos[2] == 0
    assert la2.states[2] == q_yes and la2.done[2] == 1 and st2.live[2] == 0 and la2.states[1] == q0 and la2.violated[1] == -7


# ---- one finalize kernel, two state layouts -------------------------------------------------------------------------------------------

_FIELDS = ("token", "pos", "live", "count", "limit", "n_stop")


def _two_layout_contents(vocab, cap, stride, UNT):
    """Lanes 0..7 as both layouts hold them, and a logits row per lane.  Per triple of lanes a launch touches ([0, 3) and [5, 8)):
    0 a tie (the last maximum wins) and stays live, 1 frozen, 2 at its limit; 5 picks a stop id (the last of three, in a tied row),
    6 has a full cache once the pick advances, 7 a tie and its limit.  Lanes 3 and 4 are live and never in a range."""
    rng = np.random.default_rng(vocab)
    logits = rng.standard_normal((8, vocab)).astype(np.float32)
    a, z = (2, 6) if vocab <= 8 else (5, vocab - 1)           # 2 049 tokens: the two maxima lie in different argmax blocks
    for l in (0, 5, 7):
        logits[l, a] = logits[l, z] = 9.0
    for l in (1, 2, 3, 4, 6):
        logits[l, (3 * l) % vocab] = 9.0
    lanes = []
    for l in range(8):
        s = dict(token=UNT - l, pos=10 + l, live=1, count=l % 3, limit=1 << 20, n_stop=2, stop=[vocab + 1, vocab + 2] + [UNT] * 14)
        lanes.append(s)
    lanes[1]["live"] = 0
    lanes[2]["limit"] = lanes[2]["count"] + 1
    lanes[5]["n_stop"], lanes[5]["stop"][:3] = 3, [vocab + 1, a, z]
    lanes[6]["pos"] = cap - 1
    lanes[7]["limit"] = lanes[7]["count"] + 1
    return logits, lanes


def _fill_layout(st, hist, lanes, rows, UNT):
    for l in range(rows):                                 # behind lane 7 (the 64-lane layout): live sentinels no range reaches
        s = lanes[l] if l < 8 else dict(token=UNT - l, pos=UNT, live=1, count=2, limit=UNT, n_stop=16, stop=[UNT] * 16)
        for f in _FIELDS:
            getattr(st, f)[l] = s[f]
        for e in range(16):
            st.stop[l][e] = s["stop"][e]
    hist[:] = UNT
    for l in range(8):                                    # the history rows hold earlier picks up to the lane's count
        hist[l, :lanes[l]["count"]] = 100 + l


def _read_layout(st, rows):
    return {f: [getattr(st, f)[l] for l in range(rows)] for f in _FIELDS} | {"stop": [[st.stop[l][e] for e in range(16)] for l in range(rows)]}


def _pick_rule(logits, lanes, first, n, cap, advance, stride):
    """launch_lane_pick's rule on the host: TS.last_max, then the finalize (count, pos, history, the three ways a lane ends)."""
    want, hist = [dict(s, stop=list(s["stop"])) for s in lanes], {}
    for l in range(first, first + n):
        s = want[l]
        if not s["live"]:
            continue
        tok, cnt = TS.last_max(logits[l]), s["count"]
        if 0 <= cnt < stride:
            hist[(l, cnt)] = tok
        s["count"], s["pos"] = cnt + 1, s["pos"] + (1 if advance else 0)
        if cnt + 1 >= s["limit"] or s["pos"] >= cap or tok in s["stop"][:min(s["n_stop"], 16)]:
            s["live"] = 0
        else:
            s["token"] = tok
    return want, hist


@pytest.mark.parametrize("advance", [0, 1])
@pytest.mark.parametrize("first_lane", [0, 5])
@pytest.mark.parametrize("vocab", [8, 2049])
def test_the_pick_is_one_kernel_over_both_state_layouts(vocab, first_lane, advance):
    """The same lanes 0..7 through kjarni_hip_op_lane_automaton_pick (every slot kind 0: the plain pick) in the 8-lane and in the
    64-lane layout: the same state, history rows and scratch, the host rule's, and nothing else written.  The hook itself fails a
    call whose scratch does not come back all zero or whose guard words around logits, state, history, scratch or table changed, so
    the scratch and the guards are equal between the layouts wherever both calls return."""
    from kjarni_amd import _ffi
    K = _K()
    n, stride, cap, UNT = 3, 6, 40, -77
    logits, lanes = _two_layout_contents(vocab, cap, stride, UNT)
    want, want_hist = _pick_rule(logits, lanes, first_lane, n, cap, advance, stride)
    assert TS.last_max(logits[0]) == TS.last_max(logits[5]) == lanes[5]["stop"][2] == (vocab - 1 if vocab > 8 else 6)   # the later maximum
    got = {}
    for rows, st in ((8, _ffi.KjarniHipLaneState()), (64, _ffi.KjarniHipWideState())):
        hist = np.empty((rows, stride), np.int32)
        _fill_layout(st, hist, lanes, rows, UNT)
        before, hist0 = _read_layout(st, rows), hist.copy()
        la = K.LaneAutomata([None] * 8)
        la.pick(logits[:first_lane + n], st, hist, cap, lanes=n, first_lane=first_lane, advance=advance)
        after = _read_layout(st, rows)
        in_range = (np.arange(64) >= first_lane) & (np.arange(64) < first_lane + n)              # kind 0: the automata saw nothing
        assert (la.violated == np.where(in_range, 0, -7)).all() and (la.states == 0).all() and (la.done == 0).all()
        for l in range(rows):
            exp = {f: want[l][f] for f in _FIELDS + ("stop",)} if l < 8 else {f: before[f][l] for f in before}
            assert {f: after[f][l] for f in after} == exp, f"{rows}-lane layout, lane {l}"
            exp_row = hist0[l].copy()
            for (hl, at), tok in want_hist.items():
                if hl == l:
                    exp_row[at] = tok
            assert (hist[l] == exp_row).all(), f"{rows}-lane layout, history row {l}"
        got[rows] = ({f: [after[f][l] for l in range(8)] for f in after}, hist[:8].copy())
    assert got[8][0] == got[64][0] and (got[8][1] == got[64][1]).all()
    live = [want[l]["live"] for l in range(first_lane, first_lane + n)]
    assert live == ([1, 0, 0] if first_lane == 0 else [0, 0 if advance else 1, 0])               # every way a lane ends was taken


# ---- the loops -------------------------------------------------------------------------------------------------------------------------

class _Case:
    def __init__(self, tmp, case):
        from kjarni_amd import HipDecoder
        K = _K()
        self.case = case
        self.seed, self.cfg, t, self.ps, self.news = LCC.case_set(case)
        d = str(tmp / case)
        LCC.write_model(case, self.seed, d)
        self.dec = HipDecoder(d, 0)
        self.tokens = LCC.tokens_of(case, self.cfg)
        self.stops = LCC.stops_of(self.cfg)
        self.ref = LCC.reference(case, t, self.cfg)
        hosts = self.hosts = LCC.host_automata(self.tokens, self.stops)
        self.exp, self.infos = LCC.reference_runs(case, self.cfg, t, self.ps, self.news, hosts)
        self.cov = LCC.check(case, self.infos)            # the margins and the coverage counts, asserted again
        p = LCC.patterns()
        self.dev = {"none": None, "choices": K.Constraint(p["choices"], self.tokens), "integer": K.Constraint(p["integer"], self.tokens),
                    "brackets": K.GrammarConstraint(p["brackets"], self.tokens)}
        self.automata = [self.dev[LCC.kind_of(i)] for i in range(len(self.ps))]

    def run(self, lanes, n=None, **kw):
        n = len(self.ps) if n is None else n
        return self.dec.generate_wide_constrained(self.ps[:n], self.news[:n], self.automata[:n], lanes=lanes, lane_context=CTX, **kw)

    def single(self, i, **kw):
        """Prompt i alone through the single-stream loops: (ids, result or None)."""
        a, p, m = self.automata[i], self.ps[i], self.news[i]
        K = _K()
        if a is None:
            return self.dec.generate(p, m, **kw), None
        if isinstance(a, K.GrammarConstraint):
            return self.dec.generate_grammar(a, p, m, **kw)
        return self.dec.generate_constrained(a, p, m, **kw)


_CASES = {}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    def get(case):
        if case not in _CASES:
            _CASES[case] = _Case(tmp_path_factory.mktemp("lane_constraint"), case)
        return _CASES[case]
    return get


def _check_results(c, got, n=None):
    for i, g in enumerate(got):
        x, r = c.infos[i], g["result"]
        want = LCC.expected_result(x)
        assert {k: r[k] for k in want} == want, (i, x, r)
        if x["kind"] in ("choices", "integer"):
            assert r["final_state"] == r["device_state"] == x["final_state"] and r["final_depth"] == r["device_depth"] == 0, (i, r)
        if x["kind"] == "brackets":
            q, stack = x["final_state"]
            assert (r["final_state"], r["final_depth"]) == (r["device_state"], r["device_depth"]) == (q, len(stack)), (i, r)


@pytest.mark.parametrize("case", ["llama", "gpt2"])
def test_generate_wide_constrained_equals_the_prompt_alone_and_the_reference(cases, case):
    c = cases(case)
    assert len(c.ps) == 72 and all(4 <= m <= 10 for m in c.news)
    singles = [c.single(i) for i in range(len(c.ps))]
    assert [s[0] for s in singles] == c.exp, "precondition: the single-stream loops give the float64 ids"
    for lanes in (3, 8, 9, 64, 0):
        got = c.run(lanes)
        assert [g["ids"] for g in got] == c.exp, f"lanes = {lanes}"
        _check_results(c, got)
        for i, (g, (_, res)) in enumerate(zip(got, singles)):          # the result of the prompt alone
            if res is not None:
                assert all(g["result"][k] == v for k, v in res.items()), (lanes, i, g["result"], res)
    # plain generate_wide on the same decoder afterwards: the ids it gave before the constrained calls would have been these
    plain = [c.dec.generate(p, m) for p, m in zip(c.ps, c.news)]
    assert c.dec.generate_wide(c.ps, c.news, lanes=64, lane_context=CTX) == plain
    assert c.dec.generate_wide(c.ps, c.news, lanes=8, lane_context=CTX) == plain
    assert [g["ids"] for g in c.dec.generate_wide_constrained(c.ps, c.news, None, lanes=64, lane_context=CTX)] == plain


def test_automata_that_mask_nothing_give_the_plain_ids(cases):
    c = cases("gpt2")                                     # (one stop id, without bytes: every other token has some)
    K = _K()
    tokens = CC.universal_tokens(c.cfg["vocab_size"], G.ENDOFTEXT)
    con = K.Constraint(r"(.|\n)*", tokens)
    gram = K.GrammarConstraint([("s", r"(.|\n)*")], tokens)
    plain = c.dec.generate_wide(c.ps, c.news, lanes=64, lane_context=CTX)
    for a in (con, gram):
        got = c.dec.generate_wide_constrained(c.ps, c.news, [a] * len(c.ps), lanes=64, lane_context=CTX)
        assert [g["ids"] for g in got] == plain
        assert all(g["result"]["violated"] == 0 and g["result"]["accepted"] == 1 for g in got)
    mixed = c.dec.generate_wide_constrained(c.ps[:20], c.news[:20], [con, None, gram, None] * 5, lanes=16, lane_context=CTX)
    assert [g["ids"] for g in mixed] == plain[:20]


def _clear_under_processors(c, i, penalty, ngram):
    """Is prompt i's float64 run under its mask, then the penalty, then the n-gram ban clear of GAP * P at every step?  (Another step
    kernel may reorder two logits inside the float bar: such a prompt is no fair demand of either loop.)"""
    from tests import sampled_lookup_cases as SC
    hc, V = c.hosts[LCC.kind_of(i)], c.cfg["vocab_size"]
    hist, out, cache = list(c.ps[i]), 0, c.ref.new()
    row = c.ref.logits(hist, cache)[-1]
    q = hc.start if hc else None
    while out < c.news[i]:
        legal = hc.legal(q) if hc else np.ones(V, bool)
        proc = SC.penalise(np.where(legal, row, -np.inf), hist, penalty)
        for j in range(len(hist) - ngram + 1):
            if hist[j:j + ngram - 1] == hist[len(hist) - ngram + 1:]:
                proc[hist[j + ngram - 1]] = -np.inf
        top = np.sort(proc[np.isfinite(proc)])[-2:]
        if top.size < 2 or top[1] - top[0] < LCC.GAP * SC.penalty_factor(hist, penalty):
            return False
        tok = TS.last_max(proc)
        if tok in c.stops:
            return True
        if hc:
            q = hc.step(q, tok)
            if q == CC.DEAD:
                return False
        hist.append(tok)
        out += 1
        if hc and hc.closed[q]:
            return True
        row = c.ref.logits([tok], cache)[-1]
    return True


def test_processors_under_automata_equal_the_prompt_alone(cases):
    c = cases("llama")
    keep = [i for i in range(32) if _clear_under_processors(c, i, WC.PROCESSORS["repetition_penalty"], WC.PROCESSORS["no_repeat_ngram"])]
    assert len(keep) >= 16 and {LCC.kind_of(i) for i in keep} == set(LCC.KINDS), keep
    want = [c.single(i, **WC.PROCESSORS) for i in keep]
    ps, news, auto = [c.ps[i] for i in keep], [c.news[i] for i in keep], [c.automata[i] for i in keep]
    for lanes in (8, 16):
        got = c.dec.generate_wide_constrained(ps, news, auto, lanes=lanes, lane_context=CTX, **WC.PROCESSORS)
        assert [g["ids"] for g in got] == [w[0] for w in want], lanes
        for g, (_, res) in zip(got, want):
            if res is not None:
                assert all(g["result"][k] == v for k, v in res.items()), (g["result"], res)


@pytest.mark.parametrize("top_k", [0, 4])
def test_records_under_automata_equal_generate_logprobs_alone(cases, top_k):
    c = cases("llama")
    K = _K()
    n = 20
    for lanes in (8, 16):
        got = c.run(lanes, n=n, top_k=top_k)
        assert [g["ids"] for g in got] == c.exp[:n]
        for i, g in enumerate(got):
            a = c.automata[i]
            kw = {} if a is None else dict(grammar=a) if isinstance(a, K.GrammarConstraint) else dict(constraint=a)
            one = c.dec.generate_logprobs(c.ps[i], c.news[i], top_k=top_k, **kw)
            assert one["ids"] == g["ids"]
            # (the lanes' step and the single-stream step sum in other orders: twice the float bar of the record tests, 2 * 2 * 1e-4,
            # at its smallest, as test_gpu_gen_logprobs.py compares the same two loops)
            assert np.allclose(g["logprob"], one["logprob"], atol=4e-4, rtol=0) and np.allclose(g["topk_logprob"], one["topk_logprob"], atol=4e-4, rtol=0)
            assert g["topk_ids"].shape == one["topk_ids"].shape == (len(g["ids"]), top_k)
            assert g["logprob"].shape == (len(g["ids"]),) and np.isfinite(g["logprob"]).all()


def test_a_callback_cancels_one_constrained_prompt(cases):
    c = cases("llama")
    n = 12
    victim = next(i for i in range(n) if c.infos[i]["kind"] == "brackets" and len(c.exp[i]) >= 4)
    count = [0] * n

    def cancel(i, t):
        count[i] += 1
        return not (i == victim and count[i] == 2)
    got = c.run(12, n=n, on_token=cancel)
    ids = [g["ids"] for g in got]
    assert ids[victim] == c.exp[victim][:2] and ids[:victim] + ids[victim + 1:] == c.exp[:victim] + c.exp[victim + 1:n]
    r = got[victim]["result"]
    assert r["complete"] == 0 and r["violated"] == 0 and (r["device_state"], r["device_depth"]) == (r["final_state"], r["final_depth"])
    hg = GC.HostGrammar(c.dev["brackets"].grammar, c.tokens, c.stops)
    q, stack = hg.config_after(c.exp[victim][:2])
    assert (r["final_state"], r["final_depth"]) == (q, len(stack))


def test_prefix_reuse_under_automata(cases):
    c = cases("llama")
    prefix = np.random.default_rng(77).integers(54, c.cfg["vocab_size"], 24).tolist()
    n = 20
    ps, news, auto = [prefix + p[:12] for p in c.ps[:n]], c.news[:n], c.automata[:n]
    off = c.dec.generate_wide_constrained(ps, news, auto, lanes=16, lane_context=CTX)
    c.dec.set_prefix_reuse(True)
    try:
        c.dec.reset()
        r0, c0 = c.dec.prefix_stats()
        on = c.dec.generate_wide_constrained(ps, news, auto, lanes=16, lane_context=CTX)
        r1, c1 = c.dec.prefix_stats()
    finally:
        c.dec.set_prefix_reuse(False)
    assert [g["ids"] for g in on] == [g["ids"] for g in off] and [g["result"] for g in on] == [g["result"] for g in off]
    assert c1 - c0 == 24 + sum(len(p) - 24 for p in ps) and r1 - r0 == 24 * n
    K = _K()
    for i in (1, 2, 3):                                   # a pattern, the integer, the grammar: the prompt alone
        a = auto[i]
        one = c.dec.generate_grammar(a, ps[i], news[i]) if isinstance(a, K.GrammarConstraint) else c.dec.generate_constrained(a, ps[i], news[i])
        assert one[0] == off[i]["ids"]


def test_a_gguf_model_at_eight_lanes(tmp_path):
    from kjarni_amd import HipDecoder
    from tests import gguf_fixture as GG
    K = _K()
    path = str(tmp_path / "q" / "model.gguf")
    qcfg, _ = GG.gguf_model(path, GG.LLAMA_Q, dict.fromkeys(("embed", "q", "k", "v", "o", "gate", "up", "down"), 8), seed=3, rope_freqs=True)
    dec = HipDecoder(str(tmp_path / "q"))
    tokens = GC.model_tokens(qcfg["vocab_size"])
    con, gram = K.Constraint(K.integer(), tokens), K.GrammarConstraint(GC.rules_of(GC.BRACKETS), tokens)
    ps = LC.prompts(3, qcfg["vocab_size"], n=12)
    auto = [con, gram, None] * 4
    got = dec.generate_wide_constrained(ps, 5, auto, lanes=8, lane_context=64)
    for g, a, p in zip(got, auto, ps):
        one = (dec.generate(p, 5), None) if a is None else dec.generate_grammar(a, p, 5) if a is gram else dec.generate_constrained(a, p, 5)
        assert g["ids"] == one[0]
        assert one[1] is None or all(g["result"][k] == v for k, v in one[1].items())
    from kjarni_amd._ffi import KjarniException
    with pytest.raises(KjarniException):                  # above eight lanes a quantized checkpoint stays refused
        dec.generate_wide_constrained(ps, 5, auto, lanes=9, lane_context=64)


def test_the_moe_fixture_at_sixteen_lanes(tmp_path):
    from kjarni_amd import HipDecoder
    from tests import moe_fixture as M
    K = _K()
    d = str(tmp_path / "moe")
    cfg, t = M.moe_model(d, M.MOE_SMALL)
    dec = HipDecoder(d, 0)
    ps = WC.moe_prompts(cfg["vocab_size"])
    stop = cfg["eos_token_id"] if isinstance(cfg["eos_token_id"], int) else cfg["eos_token_id"][0]
    tokens = CC.universal_tokens(cfg["vocab_size"], stop)
    con = K.Constraint(r"(.|\n)*", tokens)                # masks nothing: the ids are the float64 run's, clear at every routed token
    gram = K.GrammarConstraint([("s", r"(.|\n)*")], tokens)
    want = [WC.moe_clear_greedy(t, cfg, p, f"prompt {i}") for i, p in enumerate(ps)]
    got = dec.generate_wide_constrained(ps, WC.MOE_NEW, [con, gram, None, con] * 5, lanes=16, lane_context=CTX)
    assert [g["ids"] for g in got] == want
    assert all(g["result"]["violated"] == 0 for g in got)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_prompt_and_touch_nothing(cases, tmp_path):
    from kjarni_amd._ffi import KjarniError, KjarniException
    c = cases("llama")
    K = _K()
    c.dec.reset()
    c.dec.forward(c.ps[0])
    length, resident = c.dec.cache_len(), c.dec.resident()
    ps, news = c.ps[:12], c.news[:12]
    other = K.Constraint(K.integer(), GC.model_tokens(257))                                  # another vocabulary
    stuck = K.Constraint("q", c.tokens)                                                     # no token of the table spells it
    assert not any(t == b"q" for t in c.tokens)
    for width in (12, 4):
        for bad, word in ((other, "vocabulary"), (stuck, "allows no token")):
            auto = list(c.automata[:12])
            auto[5] = bad
            with pytest.raises(KjarniException) as e:
                c.dec.generate_wide_constrained(ps, news, auto, lanes=width, lane_context=CTX)
            assert e.value.code == KjarniError.INVALID_CONFIG and word in e.value.message and "prompt 5" in e.value.message, e.value.message
    # seventeen stop ids: the refusal of the lanes, named by prompt, ahead of the automaton's own
    from kjarni_amd import HipDecoder
    d17 = str(tmp_path / "stops17")
    LCC.synth.llm_model(d17, dict(LCC.case_config("llama"), eos_token_id=list(range(40, 57))), seed=1)
    many = HipDecoder(d17, 0)
    with pytest.raises(KjarniException) as e:
        many.generate_wide_constrained(ps, news, c.automata[:12], lanes=12, lane_context=CTX)
    assert e.value.code == KjarniError.INVALID_CONFIG and "16 stop ids" in e.value.message and "prompt 0" in e.value.message
    # both a pattern and a grammar for one prompt: through the C entry
    import ctypes as C

    from kjarni_amd import _ffi
    n = 12
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32) for p in ps]))
    off = (C.c_size_t * (n + 1))(*np.concatenate([[0], np.cumsum([len(p) for p in ps])]).tolist())
    new = (C.c_size_t * n)(*news)
    out, n_out = np.full((n, 10), 99, np.uint32), (C.c_size_t * n)(*[7] * n)
    cons, grams = (C.c_void_p * n)(), (C.c_void_p * n)()
    cons[7], grams[7] = c.dev["integer"]._h.value, c.dev["brackets"]._h.value
    res = (_ffi.KjarniHipLaneAutomatonResult * n)()
    res[7].kind = 9
    code = _ffi.lib().kjarni_hip_decoder_generate_wide_constrained(c.dec._h, flat.ctypes.data_as(C.POINTER(C.c_uint32)), off, n, new, 1.0, 0, 12, CTX,
                                                                  _ffi.KjarniBatchTokenCallbackFn(), None, out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                                  10, n_out, -1, None, None, None, cons, grams, res)
    assert code == KjarniError.INVALID_CONFIG and "not both" in _ffi.last_error() and "prompt 7" in _ffi.last_error()
    assert (out == 99).all() and res[7].kind == 9
    assert c.dec.cache_len() == length and c.dec.resident() == resident


# ---- Generator.generate_batch ---------------------------------------------------------------------------------------------------------

TEXTS = ["The quick brown fox jumps over the lazy dog", "Hello", "Once upon a time there was a small", "1 2 3 4 5 6 7 8 9",
         "In a hole in the ground there lived"]


@pytest.mark.parametrize("wide", [0, 64])
def test_generator_generate_batch_is_constrained(tmp_path, wide):
    from kjarni_amd import Generator
    from kjarni_amd.chat import GenerationConfig
    K = _K()
    d = str(tmp_path / "gpt2")
    G.gpt2_model(d, G.gpt2_config(**dict(G.SMALL, n_ctx=128)), seed=4, tokenizer=True)
    gen = Generator("gpt2", model_path=d)
    texts = [f"{t} {i}" for i in range(4) for t in TEXTS]                                   # 20 texts: 8 lanes turn over
    greedy = GenerationConfig(do_sample=False, max_new_tokens=12)
    if wide:
        gen.set_wide_lanes(wide)
    else:
        gen.set_lanes(8)
    plain = gen.generate_batch(texts, greedy)
    assert gen.batch_constraint_result(0)["kind"] == 0
    pattern = K.choices(["yes", "no", "maybe so"])
    gen.set_constraint(pattern)
    got = gen.generate_batch(texts, greedy)
    assert all(re.fullmatch(pattern, g) for g in got), got                                 # (fails where generate_batch ignores the pattern)
    for i, g in enumerate(got):
        r = gen.batch_constraint_result(i)
        assert r["kind"] == 1 and r["complete"] == 1 and r["accepted"] == 1 and r["violated"] == 0 and r["device_state"] == r["final_state"]
        assert g == gen.generate(texts[i], greedy)
    assert gen.batch_constraint_result(len(texts))["kind"] == 0
    gen.set_constraint(None)                                                                # the plain texts again
    assert gen.generate_batch(texts, greedy) == plain
    assert gen.batch_constraint_result(0)["kind"] == 0
    gen.set_grammar(K.json_value())
    got = gen.generate_batch(texts, greedy)
    complete = 0
    for i, g in enumerate(got):
        r = gen.batch_constraint_result(i)
        assert r["kind"] == 2 and r["violated"] == 0 and (r["device_state"], r["device_depth"]) == (r["final_state"], r["final_depth"])
        if r["complete"]:
            json.loads(g)
            complete += 1
        assert g == gen.generate(texts[i], greedy)
    print("complete JSON documents:", complete, "of", len(got))
    gen.set_grammar(None)
    assert gen.generate_batch(texts, greedy) == plain
    assert gen.batch_constraint_result(0)["kind"] == 0
    # seeded sampling under the pattern: the same texts at widths 16 and 64, every one a full match
    gen.set_constraint(pattern)
    hot = GenerationConfig(do_sample=True, temperature=1.5, max_new_tokens=12)
    runs = []
    for lanes in (16, 64):
        gen.set_wide_lanes(lanes)
        gen.seed(1234)
        runs.append(gen.generate_batch(texts, hot))
    assert runs[0] == runs[1] and all(re.fullmatch(pattern, g) for g in runs[0])
    # ... and equal to the prompt alone with the same draws: every prompt of a batch draws from a generator of its own, whose seed the
    # handle reports; the single-stream loop (mask, the device's cut, the host's draw) under that seed is the independent reference
    seeds = [gen.batch_seed(i) for i in range(len(texts))]
    assert len(set(seeds)) > 1 and all(s > 0 for s in seeds) and gen.batch_seed(len(texts)) == 0
    for i, text in enumerate(texts):
        gen.seed(seeds[i])
        assert gen.generate(text, hot) == runs[0][i], i
    assert len(set(runs[0])) > 1, "the draws decide nothing"
    # the same under the grammar, penalty and all (the slow path: mask, processors, the host's draw, the device automaton follows)
    gen.set_grammar(K.json_value())
    hot2 = GenerationConfig(do_sample=True, temperature=1.2, repetition_penalty=1.2, max_new_tokens=12)
    gen.set_wide_lanes(16)
    gen.seed(99)
    batch = gen.generate_batch(texts, hot2)
    seeds = [gen.batch_seed(i) for i in range(len(texts))]
    for i, text in enumerate(texts):
        r = gen.batch_constraint_result(i)
        assert r["violated"] == 0 and (r["device_state"], r["device_depth"]) == (r["final_state"], r["final_depth"]), (i, r)
        gen.seed(seeds[i])
        assert gen.generate(text, hot2) == batch[i], i
        assert gen.grammar_result()["final_state"] == r["final_state"] and gen.grammar_result()["final_depth"] == r["final_depth"]
