"""The output stage's silence step, host side: the symbols, the refusals, hold and bound — and the definition
restated in numpy float32 (hop energies in the stated order, runs, seam), which q3_silence_trim must reproduce BITWISE, with the
streaming rule restated twice: as the number of complete hops each kept hop waits for, and as a state machine that walks the pushes.
The `gpu` tests of test_silence_stage.py import the restatement and hold the device to it. No GPU here."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api

NEW = ["q3_pcm_stage_set_silence", "q3_pcm_stage_silence", "q3_pcm_stage_silence_hold", "q3_pcm_stage_bound_silence", "q3_silence_trim",
       "q3_session_set_silence", "q3_session_silence", "q3_batcher_ticket_silence", "q3_batcher_ticket_silence_read"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, H, G = 24000, 240, 2
Q3_INVALID_ARG = 1
FLUSH = 1 << 60                                            # "waits for the flush" in hops
f32, f64 = np.float32, np.float64
SETTINGS = [(-5000, 0, 20), (-5000, 50, 400), (-4000, 1000, 2000), (-9000, 100, 200)]


def hops_of(edge_ms, pause_ms):
    P = pause_ms // 10
    return edge_ms // 10, P, P - P // 2, P // 2             # E, P, P1, P2


def hold_np(edge_ms, pause_ms):
    E, P, P1, P2 = hops_of(edge_ms, pause_ms)
    return (max(E, P1) + P2 + G + 2) * H


# ---------------------------------------------------------------- the signals, from seeds
def make_signal(spec, thr, seed, tail=0):
    """spec: [(kind, hops)], tail: samples of one more, partial hop of the last kind. S: Gaussian at -20 dBFS; Q: at -80 dBFS; Z: zeros;
    T: hops whose mean square is 1 mB above and below the threshold in turn. Built in float64, rounded once."""
    rng = np.random.default_rng(seed)
    out = []
    for kind, n in spec + ([(spec[-1][0], -tail)] if tail else []):
        cnt = n * H if n > 0 else -n
        g = rng.standard_normal(cnt)
        if kind == "S":
            out.append(g * 10.0 ** (-20.0 / 20.0))
        elif kind == "Q":
            out.append(g * 10.0 ** (-80.0 / 20.0))
        elif kind == "Z":
            out.append(np.zeros(cnt))
        else:
            g = g.reshape(-1, H)
            side = np.where(np.arange(g.shape[0]) % 2 == 0, 1.0, -1.0)
            want = 10.0 ** ((thr + side) / 1000.0)          # mean square of the hop
            out.append((g * np.sqrt(want / np.mean(g * g, axis=1))[:, None]).reshape(-1))
    return np.concatenate(out).astype(f32)


def main_spec(edge_ms, pause_ms):
    """a silence segment of S + 2 G hops between speech is a run of S hops (the guard takes G on each side), S + G at an end"""
    E, P, P1, P2 = hops_of(edge_ms, pause_ms)
    return [("Q", E + 1 + G), ("S", 5), ("Q", P + 2 * G), ("S", 3), ("Q", P + 1 + 2 * G), ("S", 4), ("Q", max(E, 1) + 2 * G), ("S", 1),
            ("Q", E + 1 + 2 * G), ("S", 6), ("Q", 4), ("T", 7), ("Q", 5), ("S", 2), ("Q", 2 * P + 3 + 2 * G), ("S", 5), ("Q", E + 1 + G)]


def signals(thr, edge_ms, pause_ms):
    """the signals for one setting"""
    E, P, P1, P2 = hops_of(edge_ms, pause_ms)
    gap = lambda k, S: (k, S + 2 * G)
    main = main_spec(edge_ms, pause_ms)
    return {
        "main": make_signal(main, thr, 1, tail=100),        # not a multiple of 240; starts and ends in silence
        "zeros": make_signal([(("Z" if k == "Q" else k), n) for k, n in main], thr, 2),
        "active_ends": make_signal([("S", 4), gap("Q", P + 2), ("S", 3), gap("Q", 1), ("S", 4)], thr, 3, tail=17),
        "silent": make_signal([("Q", E + 7)], thr, 4, tail=239),
        "short_silent": make_signal([("Q", max(E - 1, 1))], thr, 5),
    }


# ---------------------------------------------------------------- the definition, restated
def theta_np(thr):
    return f32(240.0 * math.pow(10.0, thr / 1000.0))


def energies(x):
    """e_h: 64 interleaved partial sums in ascending j, product and sum rounded once, folded d = 32 .. 1"""
    x = np.ascontiguousarray(x, f32)
    NH = -(-x.size // H)
    v = np.zeros(NH * H, f32); v[:x.size] = x
    v = np.where(np.isfinite(v), v, f32(0)).astype(f32)
    sq = (v * v).astype(f32).reshape(NH, H)
    p = np.zeros((NH, 64), f32)
    for j0 in range(0, H, 64):
        w = min(64, H - j0)
        p[:, :w] = (p[:, :w] + sq[:, j0:j0 + w]).astype(f32)
    d = 32
    while d >= 1:
        p[:, :d] = (p[:, :d] + p[:, d:2 * d]).astype(f32)
        d //= 2
    return p[:, 0].copy()


def classify(x, thr):
    """(loud, active) per hop"""
    with np.errstate(invalid="ignore"):
        loud = energies(x) > theta_np(thr)
    act = loud.copy()
    for k in range(1, G + 1):
        act[k:] |= loud[:-k] if loud.size > k else False
        act[:-k] |= loud[k:] if loud.size > k else False
    return loud, act


def run_list(act):
    """maximal stretches (s, S) of non-active hops"""
    out = []; s = None
    for h, a in enumerate(act):
        if not a and s is None:
            s = h
        if a and s is not None:
            out.append((s, h - s)); s = None
    if s is not None:
        out.append((s, len(act) - s))
    return out


def kept_hops(act, N, edge_ms, pause_ms):
    """The rules per run: (ops, need, counts). ops: [(hop, partner or -1)] in order; need[k]: the complete hops op k waits for under
    the streaming rule (FLUSH: the flush); counts: (n_in, n_out, lead, pause, trail)."""
    E, P, P1, P2 = hops_of(edge_ms, pause_ms)
    NH = len(act)
    fate = {}                                               # hop -> (partner, need) for the hops of runs that are kept
    lead = pause = trail = 0
    for s, S in run_list(act):
        end_need = s + S + G + 1 if s + S < NH else FLUSH    # the run ends when the active hop behind it is classified
        if s == 0:
            k = min(S, E)
            for h in range(S - k, S):
                fate[h] = (-1, end_need)
            lead = min((S - k) * H, N)
        elif s + S == NH:
            k = min(S, E)
            for i in range(k):
                fate[s + i] = (-1, s + i + G + 1 if i < min(E, P1 - 1) else FLUSH)
            trail = N - min(N, (s + k) * H)
        else:
            keep = list(range(S)) if S <= P else list(range(P1)) + list(range(S - P2, S))
            for i in keep:
                fate[s + i] = (-1, s + i + G + 1 if i < min(E, P1 - 1) else end_need)
            if S > P:
                fate[s + P1 - 1] = (s + S - P2 - 1, end_need)
                pause += (S - P) * H
    ops, need = [], []
    for h in range(NH):
        if act[h]:
            ops.append((h, -1)); need.append(h + G + 1)
        elif h in fate:
            ops.append((h, fate[h][0])); need.append(fate[h][1])
    n_out = len(ops) * H
    if ops and (ops[-1][0] + 1) * H > N:
        n_out -= (ops[-1][0] + 1) * H - N
    return ops, np.array(need, np.int64), (N, n_out, lead, pause, trail)


def seam_weights():
    t = (np.arange(H, dtype=f64) + 0.5) / 240.0
    return t.astype(f32), (1.0 - t).astype(f32)


def restate(x, thr, edge_ms, pause_ms):
    """(y, counts, ops, need): the whole definition"""
    x = np.ascontiguousarray(x, f32)
    _, act = classify(x, thr)
    ops, need, counts = kept_hops(act, x.size, edge_ms, pause_ms)
    w0, w1 = seam_weights()
    xp = np.zeros(len(act) * H, f32); xp[:x.size] = x
    parts = []
    for a, b in ops:
        xa = xp[a * H:(a + 1) * H]
        parts.append(xa if b < 0 else ((xa * w1).astype(f32) + (xp[b * H:(b + 1) * H] * w0).astype(f32)).astype(f32))
    y = np.concatenate(parts)[:counts[1]] if parts else np.zeros(0, f32)
    return y, counts, ops, need


def push_sizes(N, cut):
    sizes = [cut] * (N // cut)
    if N % cut:
        sizes.append(N % cut)
    return sizes or [0]


def stream_counts(need, counts, sizes):
    """samples each push returns (the last push carries `last`): op k leaves in the first push after which need[k] hops are complete"""
    tot = np.cumsum(np.asarray(sizes, np.int64))
    done = np.searchsorted(need, tot // H, side="right")    # ops out after each push (need is non-decreasing)
    done[-1] = need.size
    out = done * H
    out[-1] = counts[1]
    return np.diff(np.concatenate([[0], out]))


def walk_pushes(act, N, edge_ms, pause_ms, sizes):
    """The streaming rule as a state machine over the pushes: per push the samples returned and the samples the row retains
    afterwards (the hops whose fate is open or that a later seam or tail still needs, the guard and the partial hop)."""
    E, P, P1, P2 = hops_of(edge_ms, pause_ms)
    m, M = min(E, P1 - 1), max(E, P1)
    NH = len(act)
    s = -1; K = 0; tot = 0; outs = []; kept = []
    n_emit = 0; last_hop = -1
    for k, n in enumerate(sizes):
        last = k == len(sizes) - 1
        tot += n
        K1 = NH if last else max(0, tot // H - G)
        e0 = n_emit
        for h in range(K, K1):
            if act[h]:
                if s >= 0:
                    S = h - s
                    if s == 0:
                        n_emit += min(S, E)
                    elif S <= P:
                        n_emit += S - min(S, m)
                    else:
                        n_emit += P - m
                    s = -1
                n_emit += 1; last_hop = h
            else:
                if s < 0:
                    s = h
                if s > 0 and h - s < m:
                    n_emit += 1; last_hop = h
        if last and s >= 0:
            S = NH - s; k_ = min(S, E)
            n_emit += k_ if s == 0 else k_ - min(S, m)
            if k_ > 0 and (s == 0 or k_ > min(S, m)):
                last_hop = (NH - 1) if s == 0 else s + k_ - 1
            s = -1
        K = K1
        o = (n_emit - e0) * H
        if last and last_hop == NH - 1 and NH * H > N and n_emit > 0:
            o -= NH * H - N
        outs.append(o)
        held = tot - K * H if not last else 0                # the guard's complete hops and the partial one
        if s == 0:
            held += min(K - s, E) * H
        elif s > 0:
            S = K - s
            front = set(range(min(S, m), min(S, M)))
            held += len(front | set(range(max(0, S - (P2 + 1)), S)) - set(range(min(S, m)))) * H
        kept.append(held)
    return np.array(outs, np.int64), np.array(kept, np.int64)


@functools.lru_cache(maxsize=None)
def case(name, setting):
    """(x, y, counts, ops, need, act) of one signal at one setting, computed once"""
    x = signals(*setting)[name]
    y, counts, ops, need = restate(x, *setting)
    _, act = classify(x, setting[0])
    for a in (x, y, need, act):
        a.setflags(write=False)
    return x, y, counts, ops, need, act


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def trim_c(x, thr, edge_ms, pause_ms, cap=None):
    x = np.ascontiguousarray(x, f32)
    y = np.zeros(max(x.size, 1) if cap is None else max(cap, 1), f32)
    n = ctypes.c_size_t(); c = (ctypes.c_int64 * 5)()
    st = _lib.lib.q3_silence_trim(x.ctypes.data_as(ctypes.c_void_p), x.size, thr, edge_ms, pause_ms, y.ctypes.data_as(ctypes.c_void_p),
                                  x.size if cap is None else cap, ctypes.byref(n), c)
    return st, y[:n.value].copy(), tuple(int(v) for v in c)


# ---------------------------------------------------------------- the tests
def test_symbols_are_exported_bound_documented_and_in_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    shim = open(os.path.join(ROOT, "shim", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
        assert f"`{n}`" in doc, n
        assert f"fn {n}(" in shim, n
        assert f" {n}(" in hdr, n


def test_refusals():
    L = _lib.lib
    n = ctypes.c_size_t()
    for e, p in ((-10, 400), (1010, 400), (55, 400), (50, 10), (50, 2010), (50, 405), (50, 0)):
        assert L.q3_pcm_stage_silence_hold(e, p, ctypes.byref(n)) == Q3_INVALID_ARG, (e, p)
        assert L.q3_pcm_stage_bound_silence(24000, 1000, 0, 0, e, p, 100, ctypes.byref(n)) == Q3_INVALID_ARG, (e, p)
        assert trim_c(np.zeros(10, f32), -5000, e, p)[0] == Q3_INVALID_ARG, (e, p)
    assert L.q3_pcm_stage_silence_hold(50, 400, None) == Q3_INVALID_ARG
    assert L.q3_pcm_stage_bound_silence(24000, 1000, 0, 0, 50, 400, 100, None) == Q3_INVALID_ARG
    assert L.q3_pcm_stage_bound_silence(1234, 1000, 0, 0, 50, 400, 100, ctypes.byref(n)) != 0
    for thr in (-9001, -1999, 100, 0):                      # (0 is off: nothing for the host function to do)
        assert trim_c(np.zeros(10, f32), thr, 50, 400)[0] == Q3_INVALID_ARG, thr
    x = np.zeros(480, f32)
    assert L.q3_silence_trim(None, 480, -5000, 50, 400, None, 0, ctypes.byref(n), None) == Q3_INVALID_ARG
    assert L.q3_silence_trim(x.ctypes.data_as(ctypes.c_void_p), 480, -5000, 50, 400, None, 0, None, None) == Q3_INVALID_ARG
    assert L.q3_silence_trim(x.ctypes.data_as(ctypes.c_void_p), 480, -5000, 50, 400, None, 0, ctypes.byref(n), None) == 0 and n.value == 480
    assert L.q3_silence_trim(x.ctypes.data_as(ctypes.c_void_p), 480, -5000, 50, 400, None, 10, ctypes.byref(n), None) == Q3_INVALID_ARG
    assert trim_c(x, -5000, 50, 400, cap=479)[0] == Q3_INVALID_ARG
    # a null stage is refused before anything else
    assert L.q3_pcm_stage_set_silence(None, 0, -5000, 50, 400) == Q3_INVALID_ARG
    assert L.q3_pcm_stage_silence(None, 0, None, None, None, None, None) == Q3_INVALID_ARG
    assert b"silence" in L.q3_last_error()


def test_hold_and_bound_against_the_restatement():
    n = ctypes.c_size_t()
    for e in (0, 10, 50, 500, 1000):
        for p in (20, 30, 40, 400, 1990, 2000):
            assert api.pcm_stage_silence_hold(e, p) == hold_np(e, p)
            for rate, tempo, cents, lvl, n_in in ((24000, 1000, 0, False, 1920), (16000, 1250, 0, True, 19200), (8000, 1000, 300, False, 1)):
                assert api.pcm_stage_bound(rate, n_in, tempo, lvl, cents, silence=(e, p)) == api.pcm_stage_bound(rate, n_in + hold_np(e, p), tempo, lvl, cents)
    assert hold_np(1000, 2000) == 48960 == 204 * H


@pytest.mark.parametrize("setting", SETTINGS)
def test_host_function_is_the_restatement_bitwise(setting):
    cut_somewhere = False
    for name in signals(*setting):
        x, y, counts, ops, need, act = case(name, setting)
        st, yc, cc = trim_c(x, *setting)
        assert st == 0, _lib.lib.q3_last_error()
        assert cc == counts, (name, cc, counts)
        assert yc.size == y.size and (bits(yc) == bits(y)).all(), name
        n_in, n_out, lead, pause, trail = cc
        assert n_in - lead - pause - trail == n_out, (name, cc)
        assert (np.diff(need) >= 0).all(), name              # what waits longer never stands in front of what leaves sooner
        cut_somewhere |= n_out < n_in
        got = api.trim_silence(x, setting[0] / 100.0, setting[1], setting[2], counts=True)
        assert (bits(got[0]) == bits(y)).all() and tuple(got[1]) == counts
    assert cut_somewhere or setting[0] == -9000            # (at -90 dB the -80 dBFS silence is loud: only the zeros signal is cut)


def test_signals_hold_the_cases_the_rules_distinguish():
    thr, e_ms, p_ms = SETTINGS[1]
    E, P, P1, P2 = hops_of(e_ms, p_ms)
    x, y, counts, ops, need, act = case("main", SETTINGS[1])
    lens = [S for s, S in run_list(act)]
    assert {E + 1, P, P + 1, max(E, 1), 2 * P + 3} <= set(lens), lens
    assert x.size % H != 0 and not act[0] and not act[-1]
    loud, _ = classify(x, thr)
    spec = main_spec(e_ms, p_ms)
    t0 = sum(n for k, n in spec[:[k for k, n in spec].index("T")])
    assert loud[t0:t0 + 7].tolist() == [True, False] * 3 + [True]      # 1 mB above and below the threshold in turn
    e = energies(x)[t0:t0 + 7] / theta_np(thr)
    assert np.abs(e - 1.0).max() < 3e-3
    xa = case("active_ends", SETTINGS[1])
    assert xa[5][0] and xa[5][-1]
    assert not case("silent", SETTINGS[1])[5].any()
    # a seam hop is two products and a sum
    seams = [(a, b) for a, b in ops if b >= 0]
    assert len(seams) == 2 and all(b - a == S - P for (a, b), S in zip(seams, (P + 1, 2 * P + 3)))


def test_non_finite_samples():
    setting = SETTINGS[1]
    x = case("main", setting)[0].copy()
    E, P, P1, P2 = hops_of(*setting[1:])
    x[(E + 1 + G + 2) * H + 7] = np.nan                     # inside the first burst: kept
    x[(E + 1 + G + 3) * H + 9] = np.inf
    x[3] = np.nan                                           # inside the leading run's dropped part
    x[(E + 1 + G + 5 + G + P1 + 3) * H + 5] = -np.inf      # inside a pause
    y, counts, ops, need = restate(x, *setting)
    st, yc, cc = trim_c(x, *setting)
    assert st == 0 and cc == counts and (bits(yc) == bits(y)).all()
    assert np.isnan(yc).sum() == 1 and np.isinf(yc).sum() >= 1


def test_streaming_rule_two_restatements_agree():
    """every split of a 3 s signal into two pushes, and the cuts: the closed form (each kept hop leaves once `need` hops are complete)
    against the state machine; nothing retained beyond hold; every push within bound_silence"""
    setting = (-5000, 50, 400)
    E, P, P1, P2 = hops_of(*setting[1:])
    spec = [("Q", 12), ("S", 20), ("Q", P + 1 + 2 * G), ("S", 30), ("Q", 9), ("S", 25), ("Q", E + 1 + 2 * G), ("S", 40), ("Q", 110)]
    x = make_signal(spec, setting[0], 9, tail=60)[:3 * FS]
    assert x.size == 3 * FS
    y, counts, ops, need = restate(x, *setting)
    assert counts[1] < counts[0] and counts[2] > 0 and counts[3] > 0 and counts[4] > 0
    _, act = classify(x, setting[0])
    hold = hold_np(*setting[1:])
    N = x.size
    seen = set()
    for c in range(1, N):
        closed = stream_counts(need, counts, [c, N - c])
        assert closed.sum() == counts[1]
        # both restatements see a split through c // 240 alone (the hops that are complete after the first push): the state machine
        # walks each such value once, and again at the three places of a hop where an off-by-one would show
        if c // H in seen and c % H not in (0, 1, H - 1):
            continue
        seen.add(c // H)
        sm, held = walk_pushes(act, N, *setting[1:], [c, N - c])
        assert (sm == closed).all(), (c, sm, closed)
        assert held.max() <= hold, (c, held)
        assert closed[0] <= api.pcm_stage_bound(24000, c, silence=setting[1:])
    for cut in (1, 239, 240, 241, 1920, 5000):
        sizes = push_sizes(N, cut)
        closed = stream_counts(need, counts, sizes)
        sm, held = walk_pushes(act, N, *setting[1:], sizes)
        assert (sm == closed).all(), cut
        assert closed.sum() == counts[1] and held.max() <= hold, cut
        assert (closed <= np.array(sizes) + hold).all(), cut
        assert closed.max() <= api.pcm_stage_bound(24000, cut, silence=setting[1:]), cut
    # the rule at the limits too: the state machine never holds more than hold
    for setting2 in ((-5000, 0, 20), (-5000, 1000, 20), (-5000, 0, 2000), (-5000, 100, 200)):
        x2, _, counts2, _, need2, act2 = case("main", setting2)
        for cut in (240, 1920, 5000):
            sizes = push_sizes(x2.size, cut)
            sm, held = walk_pushes(act2, x2.size, *setting2[1:], sizes)
            assert (sm == stream_counts(need2, counts2, sizes)).all(), (setting2, cut)
            assert held.max() <= hold_np(*setting2[1:]), (setting2, cut, held.max())
