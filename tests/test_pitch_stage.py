"""The output stage's pitch step (DESIGN 4.12d, q3_pcm_stage_set_pitch and friends): a row at tempo t and c cents runs its
stretcher at te = llround(t / 2^(c / 1200)) and k_pitch resamples the stretcher's output by te / t with q3_resample's filter, its
taps interpolated from two tables. Host-only parts (the plan, the tables, the counts, the bound, the refusals, the definition
against q3_resample's formula) run anywhere; the `gpu` tests feed synthetic PCM — no model — and compare bitwise across cuts, rows
and compositions, and against a float64 evaluation of the definition on the stretcher's own output (teacher-forced: a second row
at tempo te and 0 cents delivers it)."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api

NEW = ["q3_pcm_stage_pitch_plan", "q3_pcm_stage_pitch_tables", "q3_pcm_stage_pitch_count", "q3_pcm_stage_bound_pitch", "q3_pcm_stage_set_pitch",
       "q3_session_set_pitch", "q3_batcher_ticket_pitch"]
W, HS, D = 720, 360, 240
S1, S2 = 512, 64
Q3_INVALID_ARG = 1
SETTINGS = [(1000, 1200), (1000, -1200), (1000, 200), (1000, -300), (800, -300), (1250, 386)]
A0, A1, A2, A3 = 0.35875, 0.48829, 0.14128, 0.01168


# ---------------------------------------------------------------- the definition, restated
def np_te(t, c):
    return int(np.floor(t / 2.0 ** (c / 1200.0) + 0.5))


def a_of(k, t):
    return (k * HS * t) // 1000


def need_of(k, t):
    return W if k == 0 else max(a_of(k, t), a_of(k - 1, t) + HS) + D + W


def np_tempo_count(t, n, ended):
    """samples of y after n input samples (test_tempo_stage.py::np_count)"""
    if t == 1000:
        return n
    if ended:
        return (n * 1000 + t // 2) // t
    if n < W:
        return 0
    k = max(0, (n - 2000) * 1000 // (HS * t) - 2)
    assert need_of(k, t) <= n
    while need_of(k + 1, t) <= n:
        k += 1
    return (k + 1) * HS


def np_pitch_count(t, c, n, ended):
    """24 kHz samples behind the stretcher at te and the pitch step: the resampler's rule with L / M = te / t."""
    te = np_te(t, c)
    y = np_tempo_count(te, n, ended)
    if te == t:
        return y
    if ended:
        return (2 * y * te + t) // (2 * t)
    return 0 if y <= 64 else -((-(y - 64) * te) // t)


def np_tables():
    m = np.arange(61 * S1 + 2, dtype=np.float64)
    xs = np.pi * m / S1
    sc = np.where(m == 0, 1.0, np.sin(xs) / np.where(m == 0, 1.0, xs))
    v = np.arange(64 * S2 + 2, dtype=np.float64) / (64 * S2)
    w = A0 + A1 * np.cos(np.pi * v) + A2 * np.cos(2 * np.pi * v) + A3 * np.cos(3 * np.pi * v)
    return sc.astype(np.float32), np.where(v >= 1.0, 0.0, w * w).astype(np.float32)


def tap_terms(t, te, r, sc, w2):
    """For phases r (array): the lerped tables in f64 over k = -63 .. 64: s, w, and the table differences d1, d2 ([len(r)][128])."""
    k = np.arange(-63, 65, dtype=np.int64)[None, :]
    q = np.abs(np.asarray(r, np.int64)[:, None] - k * te)
    n1 = 19 * q * S1; den1 = 20 * max(t, te)
    m1 = n1 // den1; f1 = (n1 - m1 * den1) / den1
    n2 = q * S2
    m2 = n2 // te; f2 = (n2 - m2 * te) / te
    s0 = sc[m1].astype(np.float64); d1 = sc[m1 + 1].astype(np.float64) - s0
    w0 = w2[m2].astype(np.float64); d2 = w2[m2 + 1].astype(np.float64) - w0
    return s0 + f1 * d1, w0 + f2 * d2, d1, d2


def h_exact(t, te, r):
    """q3_resample's weights (q3_io.cpp) at tau = r / te - k, in f64."""
    k = np.arange(-63, 65, dtype=np.float64)[None, :]
    u = np.asarray(r, np.float64)[:, None] / te - k
    v = u / 64.0
    fc = 0.95 * min(1.0, te / t)
    w = A0 + A1 * np.cos(np.pi * v) + A2 * np.cos(2 * np.pi * v) + A3 * np.cos(3 * np.pi * v)
    w = np.where((v <= -1.0) | (v >= 1.0), 0.0, w * w)
    return fc * np.sinc(fc * u) * w


def restate(y, t, te, n_out, sc, w2):
    """The definition on the stream y in f64: (v64, B) with B the per-sample bound of the f32 evaluation."""
    fc = 0.95 * min(1.0, te / t); fcf = float(np.float32(fc))
    yz = np.concatenate([np.zeros(64), y.astype(np.float64), np.zeros(2 * 64 + 4)])
    v = np.zeros(n_out); B = np.zeros(n_out)
    for j0 in range(0, n_out, 4096):
        j = np.arange(j0, min(n_out, j0 + 4096), dtype=np.int64)
        cj = (j * t) // te; r = j * t - cj * te
        s, w, d1, d2 = tap_terms(t, te, r, sc, w2)
        idx = np.minimum(cj[:, None] + np.arange(1, 129)[None, :], yz.size - 1)      # input cj + k at yz[cj + k + 64]
        x = yz[idx]
        v[j] = fcf * np.sum(s * w * x, axis=1)
        B[j] = 2.0 ** -24 * fc * np.sum((40 * np.abs(s * w) + 2 * np.abs(w * d1) + 2 * np.abs(s * d2)) * np.abs(x), axis=1)
    return v, B


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(api.PcmStage.set_pitch) and callable(api.Session.set_pitch) and callable(api.Batcher.ticket_pitch)
    assert callable(api.pcm_stage_pitch_plan) and callable(api.pcm_stage_pitch_tables) and callable(api.pcm_stage_pitch_count)


def test_pitch_plan_matches_restatement():
    for t in (500, 800, 1000, 1250, 2000):
        for c in (-1200, -300, -1, 0, 1, 200, 386, 1200):
            te = np_te(t, c)
            if 500 <= te <= 2000:
                got, cents = api.pcm_stage_pitch_plan(t, c)
                assert got == te, (t, c)
                assert cents == pytest.approx(1200.0 * np.log2(t / te), abs=1e-9)
                assert abs(cents - c) <= 1.8, (t, c, cents)        # half a permille of te is at most 0.87 cents at te = 1000, 1.73 at 500
                if c == 0:
                    assert got == t and cents == 0.0
            else:
                with pytest.raises(_lib.Q3Error) as e:
                    api.pcm_stage_pitch_plan(t, c)
                assert e.value.status == Q3_INVALID_ARG and "stretcher" in str(e.value), (t, c)
    assert api.pcm_stage_pitch_plan(1250, 386)[0] == 1000      # the pitch step alone


def test_pitch_refusals_before_the_device():
    L = _lib.lib
    sz = ctypes.c_size_t(); te = ctypes.c_int(); cr = ctypes.c_double()
    for t, c in ((1000, 1201), (1000, -1201), (499, 0), (2001, 100), (500, 200), (2000, -300), (800, 1200)):
        assert L.q3_pcm_stage_pitch_plan(t, c, ctypes.byref(te), ctypes.byref(cr)) == Q3_INVALID_ARG and L.q3_last_error()
        assert L.q3_pcm_stage_pitch_count(t, c, 1000, 0, ctypes.byref(sz)) == Q3_INVALID_ARG and L.q3_last_error()
        assert L.q3_pcm_stage_bound_pitch(16000, t, c, 0, 1000, ctypes.byref(sz)) == Q3_INVALID_ARG and L.q3_last_error()
    assert L.q3_pcm_stage_pitch_plan(1000, 1201, None, None) == Q3_INVALID_ARG and b"cents" in L.q3_last_error()
    assert L.q3_pcm_stage_bound_pitch(47999, 1000, 200, 0, 1000, ctypes.byref(sz)) == 7      # the rate's refusal stays Q3_UNSUPPORTED
    for f in (lambda: L.q3_pcm_stage_set_pitch(None, 0, 200), lambda: L.q3_session_set_pitch(None, 0, 200),
              lambda: L.q3_batcher_ticket_pitch(None, 1, 200), lambda: L.q3_pcm_stage_pitch_count(1000, 200, 10, 0, None)):
        assert f() == Q3_INVALID_ARG and L.q3_last_error()
    assert L.q3_pcm_stage_pitch_tables(ctypes.c_void_p(1), 10, None, 0, None, None) == Q3_INVALID_ARG      # a buffer too small


def test_tables_match_numpy_to_one_ulp():
    sc, w2, s1, s2 = api.pcm_stage_pitch_tables()
    assert (s1, s2) == (S1, S2) and sc.size == 61 * S1 + 2 and w2.size == 64 * S2 + 2
    nsc, nw2 = np_tables()
    for got, want in ((sc, nsc), (w2, nw2)):
        ulp = np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    assert sc[0] == 1.0 and w2[0] == 1.0 and w2[64 * S2] == 0.0 and w2[64 * S2 + 1] == 0.0


@pytest.mark.parametrize("t,c", SETTINGS + [(1000, 0), (1250, 0), (500, -1200)])
def test_pitch_count_matches_the_rule(t, c):
    prev = 0
    for n in list(range(0, 6001, 7)) + [36000, 40000, 10 ** 6, 2 ** 31 + 12345]:
        got = api.pcm_stage_pitch_count(t, c, n); flushed = api.pcm_stage_pitch_count(t, c, n, True)
        assert got == np_pitch_count(t, c, n, False) and flushed == np_pitch_count(t, c, n, True), (t, c, n)
        assert got <= flushed, (t, c, n)                            # a flush never takes samples back
        if n <= 6000:
            assert got >= prev, (t, c, n)
            prev = got
        assert abs(flushed - np_tempo_count(t, n, True)) <= 2, (t, c, n)      # the duration is the one of the tempo


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
def test_bound_pitch_covers_every_split(sr):
    """q3_pcm_stage_bound_pitch >= what either push returns, for every split of 40000 samples into two pushes, the second flushed."""
    N = 40000
    for t, c in SETTINGS:
        for lv in (False, True):
            def total(n, ended):
                v = np_pitch_count(t, c, n, ended)
                if lv:
                    v = v if ended else max(0, v - 127)
                return n_emitted(sr, v, ended)
            end = total(N, True)
            for n0 in list(range(0, N + 1, 97)) + [1, 63, 64, 65, 127, 128, 129, 719, 720, 721, N - 1, N]:
                first = total(n0, False)
                assert api.pcm_stage_bound(sr, n0, t, lv, c) >= first, (sr, t, c, lv, n0)
                assert api.pcm_stage_bound(sr, N - n0, t, lv, c) >= end - first, (sr, t, c, lv, n0)
            # ... and not a loose one: the stretcher's hold-back (at most 1320 input samples), the 64 of each resampler, the level's 127
            te = np_te(t, c)
            slack = ((1320 * 1000 // te + 70) * te // t + 200) * sr // 24000 + 16
            assert api.pcm_stage_bound(sr, 1920, t, lv, c) <= 1920 * 1000 // t * sr // 24000 + slack, (sr, t, c, lv)


PAIRS = [(1000, 500), (1000, 501), (1000, 891), (1000, 1189), (1000, 2000), (1250, 1000), (2000, 1999), (800, 673)]


@pytest.mark.parametrize("t,te", PAIRS)
def test_definition_against_the_projects_filter(t, te):
    """For every phase r: sum over the 128 taps of |h_table - h_exact| <= 1e-5, h_table from the library's f32 tables lerped in f64,
    h_exact q3_resample's formula. (Worst over these pairs with S1 = 512, S2 = 64: 5.6e-6.)"""
    sc, w2, _, _ = api.pcm_stage_pitch_tables()
    r = np.arange(te)
    s, w, _, _ = tap_terms(t, te, r, sc, w2)
    fc = 0.95 * min(1.0, te / t)
    err = np.sum(np.abs(fc * s * w - h_exact(t, te, r)), axis=1)
    print(f"(t, te) = ({t}, {te}): worst sum |h_table - h_exact| = {err.max():.3g} at r = {int(err.argmax())}")
    assert err.max() <= 1e-5, (t, te, err.max())


# ---------------------------------------------------------------- GPU, synthetic PCM, no model
def speech_like():
    """(test_tempo_stage.py::speech_like)"""
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


def run_row(ps, row, x, piece):
    """x to `row` in pushes of `piece` samples, the last one flushed."""
    out = []; at = 0
    while True:
        n = min(piece, x.size - at); last = at + n >= x.size
        out.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
        if last:
            break
    return np.concatenate(out)


def setup(ps, row, t, c, sr=24000, s16=False):
    """(the pitch first goes back to 0: the row's old one need not admit the new tempo)"""
    ps.set(row, sr, s16); ps.set_pitch(row, 0); ps.set_tempo(row, t); ps.set_pitch(row, c)


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, 36000)
    yield ps
    ps.close()


@pytest.fixture(scope="module")
def whole(stage, sig):
    """Per setting, in one push of the whole signal at 24 kHz f32: (v, y) — the pitched row's output and the output of a row at
    tempo te and 0 cents, the stream the pitch step saw. Computed once, read by the tests below."""
    res = {}
    for t, c in SETTINGS:
        te = np_te(t, c)
        setup(stage, 0, t, c); setup(stage, 1, te, 0)
        v = run_row(stage, 0, sig, sig.size); y = run_row(stage, 1, sig, sig.size)
        v.setflags(write=False); y.setflags(write=False)
        res[(t, c)] = (v, y)
    setup(stage, 0, 1000, 0); setup(stage, 1, 1000, 0)
    return res


@pytest.mark.gpu
def test_bypass(stage, sig):
    """0 cents: at 24 kHz f32 a copy of the input; at 16 kHz s16 the bytes of a stage whose rows never had a pitch — for a row
    that never had one and for one that had one and has none now, with and without a tempo."""
    fresh = api.PcmStage(0, 1, 36000)
    want = {}
    for t in (1000, 1250):
        fresh.set(0, 16000, True); fresh.set_tempo(0, t)
        want[t] = run_row(fresh, 0, sig, 5000)
    fresh.close()
    stage.set(2, 24000); stage.set_tempo(2, 1000); stage.set_pitch(2, 0)
    np.testing.assert_array_equal(run_row(stage, 2, sig, 5000), sig)
    for t in (1000, 1250):
        setup(stage, 2, t, 0, 16000, True)
        got = run_row(stage, 2, sig, 5000)
        assert got.dtype == np.int16
        np.testing.assert_array_equal(got, want[t])
        setup(stage, 2, t, 200, 16000, True); stage.push({2: sig[:3000]}); stage.set_pitch(2, 0)
        np.testing.assert_array_equal(run_row(stage, 2, sig, 5000), want[t], err_msg=f"tempo {t}, a row that had a pitch")


@pytest.mark.gpu
@pytest.mark.parametrize("t,c", SETTINGS)
def test_totals(stage, sig, whole, t, c):
    """The flushed 24 kHz length is q3_pcm_stage_pitch_count's; every push returns what the counts say and no more than the
    bound; at rate sr the resampler's count of that; a further flush returns nothing."""
    v, y = whole[(t, c)]
    te = np_te(t, c)
    assert y.size == np_tempo_count(te, sig.size, True)
    assert v.size == api.pcm_stage_pitch_count(t, c, sig.size, True) == (2 * y.size * te + t) // (2 * t)
    for sr, s16 in ((24000, False), (16000, True), (44100, False)):
        setup(stage, 2, t, c, sr, s16)
        at = 0; got = 0
        for n in (1, 700, 1920, 33, 5000, 12000, 9000, 36000):
            n = min(n, sig.size - at); last = at + n >= sig.size
            z = stage.push({2: sig[at:at + n]}, last=(2,) if last else ())[2]
            at += n; got += z.size
            assert z.size <= api.pcm_stage_bound(sr, n, t, False, c)
            assert got == n_emitted(sr, api.pcm_stage_pitch_count(t, c, at, last), last), (t, c, sr, at)
            if last:
                break
        assert stage.push({2: sig[:0]}, last=(2,))[2].size == 0
        with pytest.raises(_lib.Q3Error):
            stage.push({2: sig[:10]})                      # a flushed row takes no more samples


@pytest.mark.gpu
@pytest.mark.parametrize("t,c", SETTINGS)
def test_cut_invariance_bitwise(stage, sig, whole, t, c):
    """Pushes of 1 / 63 / ... / 5000 samples against one push. Single samples over the first 4000 (a push each: the whole signal
    would take 36000 of them) against one push of those; every other size over the whole signal."""
    v, _ = whole[(t, c)]
    setup(stage, 2, t, c)
    short = run_row(stage, 2, sig[:4000], 4000)
    stage.reset(2)
    np.testing.assert_array_equal(run_row(stage, 2, sig[:4000], 1), short, err_msg="single samples")
    for piece in (63, 64, 65, 127, 128, 129, 359, 1920, 5000):
        stage.reset(2)
        np.testing.assert_array_equal(run_row(stage, 2, sig, piece), v, err_msg=f"pieces of {piece}")


@pytest.mark.gpu
@pytest.mark.parametrize("t,c", SETTINGS)
def test_against_float64_teacher_forced(sig, whole, t, c):
    """The f64 evaluation of the definition on the stretcher's own output y agrees with the kernel per sample within
    B_j = 2^-24 fc sum_k (40 |s w| + 2 |w d1| + 2 |s d2|) |x_k|: three roundings per lerp (the quotient, the difference, the fma),
    one product, 32 fmas and two joins per partial sum, one final product. And q3_resample(y, t, te) agrees within
    B_j + 1e-5 max |x|: the table's distance from the formula (test_definition_against_the_projects_filter)."""
    v, y = whole[(t, c)]
    te = np_te(t, c)
    sc, w2, _, _ = api.pcm_stage_pitch_tables()
    v64, B = restate(y, t, te, v.size, sc, w2)
    err = np.abs(v.astype(np.float64) - v64)
    frac = float(np.max(err / np.maximum(B, 1e-300)))
    print(f"(t, c) = ({t}, {c}), te = {te}: max |v - v64| / B = {frac:.3g}, max |v - v64| = {err.max():.3g}")
    assert np.all(err <= B), (t, c, int(np.argmax(err - B)), frac)
    n = ctypes.c_int64()
    ref = np.zeros(v.size + 4, np.float32)
    _lib.check(_lib.lib.q3_resample(y.ctypes.data_as(ctypes.c_void_p), y.size, t, te, ref.ctypes.data_as(ctypes.c_void_p), ref.size, ctypes.byref(n)))
    assert abs(int(n.value) - v.size) <= 1                  # (llround in f64 against the integer rule: a tie at most)
    m = min(int(n.value), v.size)
    err = np.abs(v[:m].astype(np.float64) - ref[:m].astype(np.float64))
    tol = B[:m] + 1e-5 * float(np.max(np.abs(y)))
    print(f"(t, c) = ({t}, {c}): max |v - q3_resample| = {err.max():.3g}, max over tolerance {float(np.max(err / tol)):.3g}")
    assert np.all(err <= tol), (t, c, int(np.argmax(err - tol)))


@pytest.mark.gpu
def test_sine_moves_by_the_realised_ratio(stage):
    """220 Hz, 1.5 s, +200 cents (te = 891): the FFT peak sits at 220 * 1000 / 891 Hz within one bin."""
    n = 36000
    x = (0.5 * np.sin(2.0 * np.pi * 220.0 * np.arange(n) / 24000.0)).astype(np.float32)
    assert np_te(1000, 200) == 891
    setup(stage, 2, 1000, 200)
    v = run_row(stage, 2, x, n)
    assert abs(v.size - n) <= 2
    spec = np.abs(np.fft.rfft(v.astype(np.float64) * np.hanning(v.size)))
    peak = float(np.argmax(spec)) * 24000.0 / v.size
    assert abs(peak - 220.0 * 1000.0 / 891.0) <= 24000.0 / v.size, peak


@pytest.mark.gpu
@pytest.mark.parametrize("t,c", [(1000, 200), (800, -300), (1250, 386)])
def test_composition_bitwise(stage, sig, t, c):
    """Row A at (24 kHz f32, t, c) yields v; row C at (16 kHz s16, t, c) with a level and a loudness target must equal row B, plain
    with the same level, loudness and rate, fed v in the same pieces."""
    setup(stage, 0, t, c)
    for r, (tt, cc) in ((1, (1000, 0)), (2, (t, c))):
        setup(stage, r, tt, cc, 16000, True)
        stage.set_level(r, 300, -100); stage.set_loudness(r, api.LOUD_NORMALIZE, -2300, 0)
    at = 0
    for n in (1, 700, 1920, 33, 5000, 12000, 9000, 36000):
        n = min(n, sig.size - at); last = at + n >= sig.size
        z = stage.push({0: sig[at:at + n]}, last=(0,) if last else ())[0]
        both = stage.push({1: z, 2: sig[at:at + n]}, last=(1, 2) if last else ())
        assert both[2].dtype == np.int16
        np.testing.assert_array_equal(both[2], both[1], err_msg=f"piece at {at}")
        at += n
        if last:
            break
    assert at == sig.size
    for r in (1, 2):
        stage.set_level(r, 0, 0); stage.set_loudness(r, api.LOUD_OFF)


@pytest.mark.gpu
def test_rows_are_independent(stage, sig, imp):
    """Three rows in one push sequence with different settings, rates, formats, push sizes and lengths (and a plain fourth)
    against their one-row runs."""
    cfg = {0: (1000, 200, 24000, False, 1920, sig[:20000]), 1: (1000, 0, 16000, True, 1000, sig[:9000]),
           2: (800, -300, 44100, False, 2500, imp), 3: (1250, 386, 8000, True, 4801, sig)}
    want = {}
    solo = api.PcmStage(0, 1, 36000)
    for r, (t, c, sr, s16, piece, x) in cfg.items():
        setup(solo, 0, t, c, sr, s16)
        want[r] = run_row(solo, 0, x, piece)
    solo.close()
    for r, (t, c, sr, s16, piece, x) in cfg.items():
        setup(stage, r, t, c, sr, s16)
    at = {r: 0 for r in cfg}; got = {r: [] for r in cfg}
    while any(at[r] < cfg[r][5].size for r in cfg):
        push = {}; last = []
        for r, (t, c, sr, s16, piece, x) in cfg.items():
            if at[r] >= x.size:
                continue
            n = min(piece, x.size - at[r])
            push[r] = x[at[r]:at[r] + n]; at[r] += n
            if at[r] >= x.size:
                last.append(r)
        out = stage.push(push, last=tuple(last))
        for r in push:
            got[r].append(out[r])
    for r in cfg:
        np.testing.assert_array_equal(np.concatenate(got[r]), want[r], err_msg=f"row {r}")


@pytest.mark.gpu
def test_commit_rule(stage, sig, whole):
    """A push refused for a small cap, one that lists the row twice and one to a flushed row leave every row's next output
    bit-equal to what it would have been; _set, _reset and every _set_* restart the row and keep the pitch; a refused setting
    changes nothing."""
    t, c = 800, -300
    v, _ = whole[(t, c)]
    v2, _ = whole[(1000, 200)]
    setup(stage, 3, t, c); setup(stage, 2, 1000, 200)
    a = stage.push({3: sig[:5000], 2: sig[:7000]})
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([3, 2], [sig[5000:12000], sig[7000:9000]], [False, False], cap=[10, 40000])
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([3, 2, 3], [sig[5000:7000], sig[7000:9000], sig[7000:9000]], [False, False, False])
    assert e.value.status == Q3_INVALID_ARG
    setup(stage, 1, 1000, -300); stage.push({1: sig[:100]}, last=(1,))
    with pytest.raises(_lib.Q3Error) as e:
        stage.push({3: sig[5000:7000], 2: sig[7000:9000], 1: sig[:10]})      # row 1 was flushed
    assert e.value.status == Q3_INVALID_ARG
    b = stage.push({3: sig[5000:], 2: sig[7000:]}, last=(3, 2))
    np.testing.assert_array_equal(np.concatenate([a[3], b[3]]), v)
    np.testing.assert_array_equal(np.concatenate([a[2], b[2]]), v2)
    restarts = (lambda: stage.reset(3), lambda: stage.set(3, 24000), lambda: stage.set_tempo(3, t), lambda: stage.set_pitch(3, c),
                lambda: stage.set_level(3, 0, 0), lambda: stage.set_loudness(3, api.LOUD_OFF))
    for restart in restarts:
        restart()                                          # (the row was flushed)
        stage.push({3: sig[:3000]})
        restart()                                          # ... and in mid-stream
        np.testing.assert_array_equal(run_row(stage, 3, sig, 12000), v)
    for bad in (lambda: stage.set_pitch(3, 1201), lambda: stage.set_pitch(3, 1200), lambda: stage.set_tempo(3, 2000)):
        with pytest.raises(_lib.Q3Error) as e:             # (800 at +1200 would need 400; 2000 at -300 would need 2378)
            bad()
        assert e.value.status == Q3_INVALID_ARG
    stage.reset(3)
    np.testing.assert_array_equal(run_row(stage, 3, sig, 36000), v)      # the refused settings changed nothing
    assert stage.tempo_lags(3)[1].size > 0                 # the stretcher's lags are those of te


@pytest.mark.gpu
def test_resample_gpu_with_pitch(sig, whole):
    np.testing.assert_array_equal(api.resample_gpu(sig, 24000, pitch_cents=200).samples, whole[(1000, 200)][0])
    np.testing.assert_array_equal(api.resample_gpu(sig, 24000, tempo_permille=800, pitch_cents=-300).samples, whole[(800, -300)][0])
    with pytest.raises(_lib.Q3Error):
        api.resample_gpu(sig, 24000, tempo_permille=2000, pitch_cents=-300)
