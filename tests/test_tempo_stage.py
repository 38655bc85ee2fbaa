"""The output stage's time stretcher (DESIGN 4.12a, q3_pcm_stage_set_tempo and friends): WSOLA in front of the resampler, per row.
Host-only parts (the streaming rule, the bound, the refusals) run anywhere; the `gpu` tests feed synthetic PCM — no model — and
compare bitwise across cuts, rows and compositions, and against a float64 restatement of the definition, teacher-forced: every
frame is scored in f64 from the positions the kernel chose so far."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api

NEW = ["q3_pcm_stage_set_tempo", "q3_pcm_stage_tempo_count", "q3_pcm_stage_bound_tempo", "q3_pcm_stage_tempo_lags", "q3_session_set_tempo",
       "q3_batcher_ticket_tempo"]
W, HS, D = 720, 360, 240
TEMPOS = [500, 800, 1250, 2000]
Q3_INVALID_ARG = 1


# ---------------------------------------------------------------- the streaming rule, restated
def a_of(k, t):
    return (k * HS * t) // 1000


def need_of(k, t):
    return W if k == 0 else max(a_of(k, t), a_of(k - 1, t) + HS) + D + W


def np_count(t, n, ended):
    """(frames, samples of y) after n input samples: the frames with need_k <= n; after the end ceil(N_out / Hs) and N_out."""
    if ended:
        n_out = (n * 1000 + t // 2) // t
        return -(-n_out // HS), n_out
    need = lambda k: need_of(k, t)
    if n < W:
        return 0, 0
    k = max(0, (n - 2000) * 1000 // (HS * t) - 2)      # from below (need_k <= k Hs t / 1000 + 1320), then single steps
    assert need(k) <= n
    while need(k + 1) <= n:
        k += 1
    return k + 1, (k + 1) * HS


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(api.PcmStage.set_tempo) and callable(api.PcmStage.tempo_lags) and callable(api.Session.set_tempo)
    assert callable(api.Batcher.ticket_tempo) and callable(api.pcm_stage_tempo_count)


@pytest.mark.parametrize("t", [500, 800, 1000, 1250, 1999, 2000])
def test_tempo_count_matches_restatement(t):
    f = ctypes.c_size_t(); y = ctypes.c_size_t()
    for n in list(range(0, 6001)) + [10 ** 6, 2 ** 31 - 1, 2 ** 31 + 12345, 10 ** 12]:
        for ended in (0, 1):
            assert _lib.lib.q3_pcm_stage_tempo_count(t, n, ended, ctypes.byref(f), ctypes.byref(y)) == 0
            assert (f.value, y.value) == np_count(t, n, bool(ended)), (t, n, ended)


def test_tempo_count_is_monotone_and_below_the_flush():
    """What has been computed before the end never exceeds what the flush then returns (a flush never takes samples back)."""
    for t in (500, 800, 1250, 1999, 2000):
        prev = 0
        for n in range(0, 6001, 7):
            f, y = api.pcm_stage_tempo_count(t, n)
            fe, ye = api.pcm_stage_tempo_count(t, n, True)
            assert y >= prev and y <= ye and f <= fe, (t, n)
            prev = y


def n_emitted(sr, n_in, ended):
    """The resampler's streaming rule (test_pcm_stage.py::n_emitted)."""
    import math
    g = math.gcd(sr, 24000); L, M = sr // g, 24000 // g
    if sr == 24000:
        return n_in
    if ended:
        return int(math.floor(n_in * (sr / 24000.0) + 0.5))
    return 0 if n_in <= 64 else -((-(n_in - 64) * L) // M)


@pytest.mark.parametrize("sr", [8000, 16000, 24000, 44100])
@pytest.mark.parametrize("t", [500, 800, 1000, 1250, 1999, 2000])
def test_bound_tempo_covers_every_split(sr, t):
    """q3_pcm_stage_bound_tempo(sr, t, n) >= what a push of n samples can return, wherever it falls in the row's stream and with
    or without `last` (the shape of test_pcm_stage.py::test_bound_covers_every_split)."""
    def total(n, ended):
        y = n if t == 1000 else np_count(t, n, ended)[1]
        return n_emitted(sr, y, ended)
    for n in (1, 359, 720, 1920, 19200):
        bound = api.pcm_stage_bound(sr, n, t)
        worst = 0
        for n0 in list(range(0, 4000, 3)) + [19200, 100000, 100001, 1000003]:
            before = total(n0, False)
            worst = max(worst, total(n0 + n, False) - before, total(n0 + n, True) - before)
        assert bound >= worst, (sr, t, n, bound, worst)
        # ... and not a loose one: the stretcher's hold-back (at most 1320 input samples) and the resampler's 64 at this ratio
        assert bound <= worst + (1320 * 1000 // t + 66) * sr // 24000 + 8, (sr, t, n, bound, worst)


def test_tempo_out_of_range_refused_before_the_device():
    """499 and 2001: Q3_INVALID_ARG from every entry point, a null stage included (the range is checked first where there is one)."""
    L = _lib.lib
    sz = ctypes.c_size_t()
    for t in (499, 2001, 0, -1000):
        assert L.q3_pcm_stage_tempo_count(t, 1000, 0, ctypes.byref(sz), ctypes.byref(sz)) == Q3_INVALID_ARG
        assert b"tempo" in L.q3_last_error()
        assert L.q3_pcm_stage_bound_tempo(16000, t, 1000, ctypes.byref(sz)) == Q3_INVALID_ARG
        with pytest.raises(_lib.Q3Error):
            api.pcm_stage_bound(16000, 1000, t)
    assert L.q3_pcm_stage_bound_tempo(47999, 1250, 1000, ctypes.byref(sz)) == 7      # the rate's refusal stays Q3_UNSUPPORTED
    for f in (lambda: L.q3_pcm_stage_set_tempo(None, 0, 1250), lambda: L.q3_session_set_tempo(None, 0, 1250),
              lambda: L.q3_batcher_ticket_tempo(None, 1, 1250), lambda: L.q3_pcm_stage_tempo_lags(None, 0, None, None, 0, ctypes.byref(sz))):
        assert f() == Q3_INVALID_ARG and L.q3_last_error()


# ---------------------------------------------------------------- GPU, synthetic PCM, no model
def speech_like():
    rng = np.random.default_rng(20240612)
    n = 36000
    t = np.arange(n) / 24000.0
    f0 = np.linspace(110.0, 180.0, n)
    ph = 2.0 * np.pi * np.cumsum(f0) / 24000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 9)) * 0.18 * (0.6 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t)) + 0.01 * rng.standard_normal(n)
    x[12000:14400] = 0.0
    x[20000:22000] = 0.05 * rng.standard_normal(2000)
    return x.astype(np.float32)


def impulses():
    x = np.zeros(24000, np.float32)
    x[::173] = 0.5
    return x


@pytest.fixture(scope="module")
def sig():
    return speech_like()


@pytest.fixture(scope="module")
def imp():
    return impulses()


def run_row(ps, row, x, piece, lags=True):
    """x to `row` in pushes of `piece` samples, the last one flushed: (samples, lags of all frames)."""
    out = []; lg = []; at = 0; k_next = 0
    while True:
        n = min(piece, x.size - at); last = at + n >= x.size
        out.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
        if lags:
            k0, l = ps.tempo_lags(row)
            if l.size:
                assert k0 == k_next, (k0, k_next)
                lg.append(l); k_next += l.size
        if last:
            break
    return np.concatenate(out), (np.concatenate(lg) if lg else np.zeros(0, np.int32))


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, 36000)
    yield ps
    ps.close()


@pytest.fixture(scope="module")
def whole(stage, sig):
    """One push of the whole signal per tempo at 24 kHz f32: {t: (y, lags)} — computed once, read by the tests below."""
    res = {}
    for t in TEMPOS:
        stage.set(0, 24000); stage.set_tempo(0, t)
        y, l = run_row(stage, 0, sig, sig.size)
        y.setflags(write=False); l.setflags(write=False)
        res[t] = (y, l)
    stage.set_tempo(0, 1000)
    return res


@pytest.mark.gpu
def test_bypass(stage, sig):
    """Tempo 1000: at 24 kHz f32 a copy of the input; at 16 kHz s16 the bytes of a stage whose rows never had a tempo."""
    stage.set(1, 24000); stage.set_tempo(1, 1000)
    y, l = run_row(stage, 1, sig, 5000)
    np.testing.assert_array_equal(y, sig)
    assert l.size == 0
    fresh = api.PcmStage(0, 1, 36000)
    fresh.set(0, 16000, True)
    want, _ = run_row(fresh, 0, sig, 5000, lags=False)
    fresh.close()
    stage.set_tempo(1, 1250); stage.set(1, 16000, True); stage.set_tempo(1, 1000)      # a row that had one and has none now
    got, _ = run_row(stage, 1, sig, 5000)
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("t", TEMPOS)
def test_totals(stage, sig, whole, t):
    """The flushed 24 kHz length is N_out = floor((n 1000 + t / 2) / t); at rate sr llround(N_out sr / 24000); a further flush
    returns nothing; the first Hs samples are the input's."""
    y, lags = whole[t]
    n_out = (sig.size * 1000 + t // 2) // t
    assert y.size == n_out and lags.size == -(-n_out // HS) and lags[0] == 0
    np.testing.assert_array_equal(y[:HS], sig[:HS])
    assert np.all(np.abs(lags) <= D)
    for sr, s16 in ((16000, True), (44100, False)):
        stage.set(1, sr, s16); stage.set_tempo(1, t)
        z, _ = run_row(stage, 1, sig, 7000)
        assert z.size == int(np.floor(n_out * (sr / 24000.0) + 0.5)), (t, sr)
        assert stage.push({1: sig[:0]}, last=(1,))[1].size == 0
        with pytest.raises(_lib.Q3Error):
            stage.push({1: sig[:10]})                      # a flushed row takes no more samples


@pytest.mark.gpu
@pytest.mark.parametrize("t", TEMPOS)
def test_cut_invariance_bitwise(stage, sig, whole, t):
    y, lags = whole[t]
    stage.set(1, 24000); stage.set_tempo(1, t)
    # single samples over the first 4000 (a push each: the whole signal would take 36000 of them), against one push of those
    short = run_row(stage, 1, sig[:4000], 4000)
    stage.reset(1)
    g, l = run_row(stage, 1, sig[:4000], 1)
    np.testing.assert_array_equal(l, short[1], err_msg="lags, single samples")
    np.testing.assert_array_equal(g, short[0], err_msg="samples, single samples")
    for piece in (359, 360, 361, 1199, 1200, 1920, 5000):
        stage.reset(1)
        g, l = run_row(stage, 1, sig, piece)
        np.testing.assert_array_equal(l, lags, err_msg=f"lags, pieces of {piece}")
        np.testing.assert_array_equal(g, y, err_msg=f"samples, pieces of {piece}")


# ---- the float64 restatement
def hann64():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)


def pick(s, lo):
    """The choice among candidates lo .. 240 with scores s: the largest, ties to the smallest |lag|, then the negative one."""
    d = np.arange(lo, D + 1)
    best = np.flatnonzero(s == s.max())
    order = sorted(best, key=lambda i: (abs(d[i]), d[i]))
    return int(d[order[0]])


def restate(x, t, lags):
    """Teacher-forced: frame k scored in f64 from p_{k-1} = a_{k-1} + lags[k-1]. Returns per frame (scores, lo, own pick, margin,
    whether every sample the frame can touch is an exact zero) and y64 with the per-sample bound."""
    K = lags.size
    xz = np.concatenate([x.astype(np.float64), np.zeros(K * HS * 2 + 4 * W)])      # zeros beyond the end
    w = hann64()
    y = np.zeros(K * HS); bound = np.zeros(K * HS)
    y[:HS] = xz[:HS]
    frames = []
    p_prev = 0
    for k in range(1, K):
        a = a_of(k, t)
        lo = max(-D, -a)
        T = xz[p_prev + HS:p_prev + HS + W]
        S = xz[a + lo:a + D + W]
        win = np.lib.stride_tricks.sliding_window_view(S, W)
        c = win @ T
        E = np.einsum("ij,ij->i", win, win)
        s = np.where(E > 0, c / np.sqrt(np.where(E > 0, E, 1.0)), 0.0)
        m = 4.0 * (W + 1) * 2.0 ** -24 * np.sqrt(T @ T)
        frames.append((s, lo, pick(s, lo), m, not S.any()))
        p = a + int(lags[k])
        t1 = w[HS:] * T[:HS]; t2 = w[:HS] * xz[p:p + HS]
        y[k * HS:(k + 1) * HS] = t1 + t2
        bound[k * HS:(k + 1) * HS] = 4.0 * 2.0 ** -24 * (np.abs(t1) + np.abs(t2))
        p_prev = p
    return frames, y, bound


def check_against_f64(x, t, y, lags, exact):
    frames, y64, bound = restate(x, t, lags)
    differ = 0; worst = 0.0
    for k, (s, lo, own, m, silent) in enumerate(frames, start=1):
        d = int(lags[k])
        assert lo <= d <= D, (t, k, d)
        gap = s.max() - s[d - lo]
        worst = max(worst, gap / m if m > 0 else (0.0 if gap == 0 else np.inf))
        assert gap <= m, (t, k, d, own, gap, m)
        if exact or silent:
            assert d == own, (t, k, d, own)                # the tie rule
        differ += d != own
    print(f"tempo {t}: {len(frames)} frames, {differ} differ from f64's own pick, worst gap / margin {worst:.3g}")
    assert differ <= 0.02 * len(frames), (t, differ, len(frames))
    err = np.abs(y.astype(np.float64) - y64[:y.size])
    print(f"tempo {t}: max |y - y64| / bound {np.max(err[HS:] / np.maximum(bound[HS:y.size], 1e-300)):.3g}")
    assert np.all(err <= bound[:y.size]), (t, int(np.argmax(err - bound[:y.size])))
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("t", TEMPOS)
def test_against_float64_restatement(sig, whole, t):
    y, lags = whole[t]
    frames = check_against_f64(sig, t, y, lags, exact=False)
    assert sum(1 for f in frames if f[4]) >= 1             # the zero stretch holds whole search regions: the lag there is 0
    assert any(int(lags[k]) != 0 for k in range(1, lags.size))      # ... and the search moves frames elsewhere


@pytest.mark.gpu
@pytest.mark.parametrize("t", [1250, 800])
def test_exact_ties_on_impulses(stage, imp, t):
    stage.set(2, 24000); stage.set_tempo(2, t)
    y, lags = run_row(stage, 2, imp, imp.size)
    check_against_f64(imp, t, y, lags, exact=True)
    stage.reset(2)
    g, l = run_row(stage, 2, imp, 1999)
    np.testing.assert_array_equal(l, lags); np.testing.assert_array_equal(g, y)


@pytest.mark.gpu
@pytest.mark.parametrize("sr,s16", [(16000, True), (44100, False)])
def test_composition_bitwise(stage, sig, sr, s16):
    """Row A at (24 kHz, f32, t) yields z; row C at (sr, fmt, t) must equal row B at (sr, fmt, 1000) fed z in the same pieces."""
    for t in TEMPOS:
        stage.set(0, 24000); stage.set_tempo(0, t)
        stage.set(1, sr, s16); stage.set_tempo(1, 1000)
        stage.set(2, sr, s16); stage.set_tempo(2, t)
        at = 0; pieces = [1, 700, 1920, 33, 5000, 12000, 9000, 4000, 36000]
        for n in pieces:
            n = min(n, sig.size - at); last = at + n >= sig.size
            z = stage.push({0: sig[at:at + n]}, last=(0,) if last else ())[0]
            both = stage.push({1: z, 2: sig[at:at + n]}, last=(1, 2) if last else ())
            assert both[2].dtype == (np.int16 if s16 else np.float32)
            np.testing.assert_array_equal(both[2], both[1], err_msg=f"tempo {t}, piece at {at}")
            at += n
            if last:
                break
        assert at == sig.size


@pytest.mark.gpu
def test_rows_are_independent(stage, sig, imp):
    """Four rows in one push sequence at tempos 500 / 1000 / 1250 / 2000 with different rates, formats, push sizes and lengths
    against their one-row runs."""
    cfg = {0: (500, 24000, False, 1920, sig[:20000]), 1: (1000, 16000, True, 1000, sig[:9000]),
           2: (1250, 44100, False, 2500, imp), 3: (2000, 8000, True, 4801, sig)}
    want = {}
    solo = api.PcmStage(0, 1, 36000)
    for r, (t, sr, s16, piece, x) in cfg.items():
        solo.set(0, sr, s16); solo.set_tempo(0, t)
        want[r] = run_row(solo, 0, x, piece)
    solo.close()
    for r, (t, sr, s16, piece, x) in cfg.items():
        stage.set(r, sr, s16); stage.set_tempo(r, t)
    at = {r: 0 for r in cfg}; got = {r: [] for r in cfg}; lg = {r: [] for r in cfg}
    while any(at[r] < cfg[r][4].size for r in cfg):
        push = {}; last = []
        for r, (t, sr, s16, piece, x) in cfg.items():
            if at[r] >= x.size:
                continue
            n = min(piece, x.size - at[r])
            push[r] = x[at[r]:at[r] + n]; at[r] += n
            if at[r] >= x.size:
                last.append(r)
        out = stage.push(push, last=tuple(last))
        for r in push:
            got[r].append(out[r])
            if cfg[r][0] != 1000:
                lg[r].append(stage.tempo_lags(r)[1])
    for r in cfg:
        np.testing.assert_array_equal(np.concatenate(got[r]), want[r][0], err_msg=f"row {r}")
        if cfg[r][0] != 1000:
            np.testing.assert_array_equal(np.concatenate(lg[r]), want[r][1], err_msg=f"lags of row {r}")


@pytest.mark.gpu
def test_commit_rule(stage, sig, whole):
    """A push refused for a small cap, and one that lists the row twice, leave the next valid push's samples and lags those of
    a run without them; _set, _reset and _set_tempo restart the row."""
    t = 1250
    y, lags = whole[t]
    stage.set(3, 24000); stage.set_tempo(3, t)
    a = stage.push({3: sig[:5000]})[3]
    k0a, la = stage.tempo_lags(3)
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([3], [sig[5000:12000]], [False], cap=[10])
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([3, 3], [sig[5000:7000], sig[7000:9000]], [False, False])
    assert e.value.status == Q3_INVALID_ARG
    k0, l = stage.tempo_lags(3)                            # still the last successful push's
    assert k0 == k0a == 0
    np.testing.assert_array_equal(l, la)
    b = stage.push({3: sig[5000:]}, last=(3,))[3]
    k0b, lb = stage.tempo_lags(3)
    assert k0b == la.size
    np.testing.assert_array_equal(np.concatenate([a, b]), y)
    np.testing.assert_array_equal(np.concatenate([la, lb]), lags)
    # restarts: each of them puts the row back at sample 0 and keeps the tempo
    for restart in (lambda: stage.reset(3), lambda: stage.set(3, 24000), lambda: stage.set_tempo(3, t)):
        restart()                                          # (the row was flushed)
        stage.push({3: sig[:3000]})
        restart()                                          # ... and in mid-stream
        assert stage.tempo_lags(3)[1].size == 0
        g, l = run_row(stage, 3, sig, 12000)
        np.testing.assert_array_equal(g, y); np.testing.assert_array_equal(l, lags)
    with pytest.raises(_lib.Q3Error) as e:
        stage.set_tempo(3, 2001)
    assert e.value.status == Q3_INVALID_ARG
    stage.reset(3)
    g, _ = run_row(stage, 3, sig[:8000], 8000)             # the refused setting changed nothing
    np.testing.assert_array_equal(g[:10 * HS], y[:10 * HS])


@pytest.mark.gpu
def test_resample_gpu_with_tempo(sig, whole):
    for t in (800, 2000):
        np.testing.assert_array_equal(api.resample_gpu(sig, 24000, tempo_permille=t).samples, whole[t][0])
