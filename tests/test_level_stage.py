"""The output stage's level step (DESIGN 4.12b, q3_pcm_stage_set_level and friends): a gain and a look-ahead peak limiter per row,
between the stretcher and the resampler. The definition is restated in numpy float32 — every operation rounded once, the sums
in the stage's order — and the device is held to it BITWISE. Host-only parts (the streaming rule, the bound, the coefficients,
the refusals) run anywhere; the `gpu` tests feed synthetic PCM, no model."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
from test_tempo_stage import np_count, n_emitted

NEW = ["q3_pcm_stage_set_level", "q3_pcm_stage_level_coeffs", "q3_pcm_stage_level_count", "q3_pcm_stage_bound_level",
       "q3_session_set_level", "q3_batcher_ticket_level"]
W, D = 128, 127
SETTINGS = [(1200, -100), (600, -300), (-600, -100), (2400, -100)]
CUTS = [1, 126, 127, 128, 129, 253, 254, 255, 256, 257, 1920, 5000]
N_SIG, N_ZEROS = 24000, 700
Q3_INVALID_ARG = 1
f32 = np.float32


# ---------------------------------------------------------------- the definition, restated
def level_count(n, ended):
    return n if ended else max(0, n - D)


def restate(x, g, c):
    """y of the whole stream x (ended), f32 throughout; also the share of samples over the ceiling and those the clamp moved."""
    x = np.asarray(x, f32); g = f32(g); c = f32(c)
    n = x.size
    u = g * x
    au = np.abs(u)
    over = au > c                                          # (a NaN compares false)
    r = np.ones(n, f32)
    np.divide(c, au, out=r, where=over)
    rp = np.concatenate([np.ones(D, f32), r, np.ones(D, f32)])         # r[-D .. n + D - 1]: 1 outside the stream
    m = np.lib.stride_tricks.sliding_window_view(rp, W).min(axis=1)      # m[j - D] ... : entry i is min r[i - D .. i]
    s = [np.zeros(n, f32) for _ in range(4)]
    for k in range(W):                                     # m[n - D + k] = entry n + k
        s[k & 3] = s[k & 3] + m[k:k + n]
    a = ((s[0] + s[1]) + (s[2] + s[3])) * f32(1.0 / W)
    p = u * a
    y = np.minimum(np.maximum(p, -c), c)
    assert y.dtype == np.float32 and a.dtype == np.float32
    return y, float(np.mean(over)), int(np.sum(y != p) - np.sum(np.isnan(p)))


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(api.PcmStage.set_level) and callable(api.Session.set_level) and callable(api.Batcher.ticket_level)
    assert callable(api.pcm_stage_level_coeffs) and callable(api.pcm_stage_level_count)


def test_null_handles_give_a_status_and_a_message():
    L = _lib.lib
    sz = ctypes.c_size_t()
    for f in (lambda: L.q3_pcm_stage_set_level(None, 0, 600, -100), lambda: L.q3_session_set_level(None, 0, 600, -100),
              lambda: L.q3_batcher_ticket_level(None, 1, 600, -100), lambda: L.q3_pcm_stage_level_count(10, 0, None),
              lambda: L.q3_pcm_stage_bound_level(16000, 1000, 10, None)):
        assert f() == Q3_INVALID_ARG and len(L.q3_last_error()) > 0
    assert L.q3_pcm_stage_bound_level(47999, 1000, 10, ctypes.byref(sz)) == 7      # the rate's refusal stays Q3_UNSUPPORTED


def test_out_of_range_levels_are_refused_before_the_device():
    L = _lib.lib
    g = ctypes.c_float(); c = ctypes.c_float(); sz = ctypes.c_size_t()
    for gain, ceil in ((-6001, 0), (2401, 0), (0, -2401), (0, 1), (100000, -100), (600, 100)):
        assert L.q3_pcm_stage_level_coeffs(gain, ceil, ctypes.byref(g), ctypes.byref(c)) == Q3_INVALID_ARG
        assert len(L.q3_last_error()) > 0
        with pytest.raises(_lib.Q3Error):
            api.pcm_stage_level_coeffs(gain, ceil)
    for gain, ceil in ((-6000, 0), (2400, -2400), (0, 0)):
        assert L.q3_pcm_stage_level_coeffs(gain, ceil, ctypes.byref(g), ctypes.byref(c)) == 0
    for t in (499, 2001):
        assert L.q3_pcm_stage_bound_level(16000, t, 1000, ctypes.byref(sz)) == Q3_INVALID_ARG


def test_coefficients_to_one_ulp_of_numpy():
    for gain in list(range(-6000, 2401, 37)) + [2400, 0, 1200, 600, -600]:
        for ceil in (0, -1, -100, -300, -1234, -2400):
            g, c = api.pcm_stage_level_coeffs(gain, ceil)
            wg = f32(np.power(10.0, gain / 2000.0)); wc = f32(np.power(10.0, ceil / 2000.0))
            assert abs(float(g) - float(wg)) <= float(np.spacing(wg)), (gain, g, wg)
            assert abs(float(c) - float(wc)) <= float(np.spacing(wc)), (ceil, c, wc)
    assert api.pcm_stage_level_coeffs(0, 0) == (f32(1.0), f32(1.0))


def test_level_count_matches_restatement():
    for n in list(range(0, 600)) + [1920, 24000, 2 ** 31 - 1, 2 ** 31 + 12345, 10 ** 12]:
        for ended in (False, True):
            assert api.pcm_stage_level_count(n, ended) == level_count(n, ended), (n, ended)


@pytest.mark.parametrize("sr", [8000, 24000, 44100])
@pytest.mark.parametrize("t", [500, 1000, 2000])
def test_bound_level_covers_every_split(sr, t):
    """Every split of 5 000 samples into two pushes: what each push returns, the second with and without `last`, is within
    q3_pcm_stage_bound_level of its size."""
    total = 5000
    memo = {}

    def emitted(n, ended):
        if (n, ended) not in memo:
            y = n if t == 1000 else np_count(t, n, ended)[1]
            memo[(n, ended)] = n_emitted(sr, level_count(y, ended), ended)
        return memo[(n, ended)]
    bound = {n: api.pcm_stage_bound(sr, n, t, level=True) for n in range(0, total + 1)}
    for n1 in range(0, total + 1):
        n2 = total - n1
        first = emitted(n1, False)
        assert bound[n1] >= first, (sr, t, n1)
        assert bound[n1] >= emitted(n1, True), (sr, t, n1)             # the first push may be the only one
        assert bound[n2] >= emitted(total, False) - first, (sr, t, n1)
        assert bound[n2] >= emitted(total, True) - first, (sr, t, n1)
    # the definition: q3_pcm_stage_bound(sr, Y + D), Y the stretcher's bound or n_in
    for n in (1, 127, 1920, 5000):
        y = n if t == 1000 else api.pcm_stage_bound(24000, n, t)
        assert bound[n] == api.pcm_stage_bound(sr, y + D)


# ---------------------------------------------------------------- GPU, synthetic PCM, no model
def signal():
    rng = np.random.default_rng(3)
    t = np.arange(N_SIG) / 24000.0
    x = 0.5 * np.sin(2.0 * np.pi * 180.0 * t) * (0.3 + 0.7 * np.abs(np.sin(2.0 * np.pi * 3.0 * t))) + 0.05 * rng.standard_normal(N_SIG)
    return np.concatenate([x, np.zeros(N_ZEROS)]).astype(f32)


@pytest.fixture(scope="module")
def sig():
    x = signal()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def want(sig):
    """The restatement per setting, computed once: {(gain, ceiling): (y, g, c, share over the ceiling, samples clamped)}"""
    res = {}
    for gain, ceil in SETTINGS:
        g, c = api.pcm_stage_level_coeffs(gain, ceil)
        y, _, clamped = restate(sig, g, c)
        share = float(np.mean(np.abs(g * sig[:N_SIG]) > c))
        y.setflags(write=False)
        res[(gain, ceil)] = (y, g, c, share, clamped)
    return res


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, N_SIG + N_ZEROS)
    yield ps
    ps.close()


def run_row(ps, row, x, piece, counts=None):
    out = []; at = 0
    while True:
        n = min(piece, x.size - at); last = at + n >= x.size
        out.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
        if counts is not None:
            counts.append((at, last, out[-1].size))
        if last:
            return np.concatenate(out)


@pytest.mark.gpu
@pytest.mark.parametrize("gain,ceil", SETTINGS)
def test_one_push_equals_the_restatement(stage, sig, want, gain, ceil):
    y, g, c, share, clamped = want[(gain, ceil)]
    print(f"({gain}, {ceil}): g {g!r} c {c!r}, share over the ceiling {share:.3f}, clamped {clamped} of {sig.size}")
    if gain > 0:
        assert 0.05 < share < 0.95, share                  # the limiter works and rests within the signal
    assert clamped <= 0.01 * sig.size, clamped
    stage.set(0, 24000); stage.set_level(0, gain, ceil)
    got = run_row(stage, 0, sig, sig.size)
    assert got.dtype == np.float32 and got.size == sig.size
    bad = np.flatnonzero(got.view(np.uint32) != y.view(np.uint32))
    assert bad.size == 0, (bad.size, int(bad[0]), float(got[bad[0]]), float(y[bad[0]]))
    assert float(np.max(np.abs(got))) <= float(c)
    assert np.all(got[N_SIG + D:] == 0.0)                  # the run of zeros comes out as zeros


@pytest.fixture(scope="module")
def whole(stage, sig):
    """One push of the whole signal at (+1200, -100): (24 kHz f32, 8 kHz ulaw) — computed once, read by the tests below."""
    stage.set(0, 24000); stage.set_level(0, 1200, -100)
    a = run_row(stage, 0, sig, sig.size)
    stage.set(0, 8000, fmt="ulaw")
    b = run_row(stage, 0, sig, sig.size)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("cut", CUTS)
def test_cut_invariance_bitwise(stage, sig, whole, cut):
    """Pushes of `cut` samples equal the one-push stream, in f32 at 24 kHz and in ulaw at 8 kHz, and the totals follow
    q3_pcm_stage_level_count before and after `last`."""
    for rate, fmt, k in ((24000, "f32", 0), (8000, "ulaw", 1)):
        stage.set(1, rate, fmt=fmt); stage.set_level(1, 1200, -100)
        ref = whole[k]
        counts = []
        got = run_row(stage, 1, sig, cut, counts)
        assert got.dtype == ref.dtype
        np.testing.assert_array_equal(got.view(np.uint32) if k == 0 else got, ref.view(np.uint32) if k == 0 else ref, err_msg=f"{fmt}, pushes of {cut}")
        total = 0
        for at, last, n in counts:
            total += n
            assert total == n_emitted(rate, api.pcm_stage_level_count(at, last), last), (fmt, cut, at, last)


@pytest.mark.gpu
def test_off_is_the_stage_without_levels(stage, sig):
    """A row at (0, 0) — never set, or set back after a level — returns the bits and the counts of a stage that never heard of
    levels, at 24 kHz f32 (a copy) and at 16 kHz s16."""
    def chunks(ps, row):
        out = []; at = 0
        while at < sig.size:
            n = min(1777, sig.size - at)
            out.append(ps.push({row: sig[at:at + n]}, last=(row,) if at + n >= sig.size else ())[row]); at += n
        return out
    for rate, s16 in ((24000, False), (16000, True)):
        fresh = api.PcmStage(0, 1, sig.size)
        fresh.set(0, rate, s16)
        ref = chunks(fresh, 0)
        fresh.close()
        stage.set(2, rate, s16); stage.set_level(2, 0, 0)  # explicit (0, 0) on a row that never had one
        a = chunks(stage, 2)
        stage.set_level(2, 1200, -100); stage.push({2: sig[:3000]}); stage.set_level(2, 0, 0)      # ... and after a level
        b = chunks(stage, 2)
        for got in (a, b):
            assert [g.size for g in got] == [r.size for r in ref]
            np.testing.assert_array_equal(np.concatenate(got), np.concatenate(ref))
    np.testing.assert_array_equal(np.concatenate(a), api.pcm16(api.resample_gpu(sig, 16000).samples))


@pytest.mark.gpu
def test_composition_with_tempo_and_rate(stage, sig):
    """tempo 1250 -> level (+600, -100) -> 16 kHz s16 in one row, streamed, equals the three steps as one-shot stages."""
    y = api.resample_gpu(sig, 24000, tempo_permille=1250).samples
    z = api.resample_gpu(y, 24000, gain_mb=600, ceiling_mb=-100).samples
    g, c = api.pcm_stage_level_coeffs(600, -100)
    np.testing.assert_array_equal(z.view(np.uint32), restate(y, g, c)[0].view(np.uint32))
    ref = api.resample_gpu(z, 16000, pcm16=True).samples
    stage.set(3, 16000, True); stage.set_tempo(3, 1250); stage.set_level(3, 600, -100)
    for piece in (sig.size, 1920, 333):
        stage.reset(3)
        got = run_row(stage, 3, sig, piece)
        assert got.dtype == np.int16
        np.testing.assert_array_equal(got, ref, err_msg=f"pieces of {piece}")
    np.testing.assert_array_equal(api.resample_gpu(sig, 16000, pcm16=True, tempo_permille=1250, gain_mb=600, ceiling_mb=-100).samples, ref)
    stage.set_tempo(3, 1000); stage.set_level(3, 0, 0)


@pytest.mark.gpu
def test_a_nan_moves_no_other_sample(stage, sig, whole):
    x = sig.copy(); z = sig.copy()
    for i in (5000, 5001, 12000):
        x[i] = np.nan; z[i] = 0.0
    stage.set(1, 24000); stage.set_level(1, 1200, -100)
    a = run_row(stage, 1, x, 4000)
    stage.reset(1)
    b = run_row(stage, 1, z, 4000)
    keep = np.ones(sig.size, bool); keep[[5000, 5001, 12000]] = False
    np.testing.assert_array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32))
    assert np.all(np.isnan(a[~keep]))
    assert np.any(a[:4000] != 0)


@pytest.mark.gpu
def test_commit_rule(stage, sig, whole):
    """A push refused for its cap, and one that lists the row twice, change nothing: the next push continues bitwise. _set,
    _reset and _set_tempo keep the level and restart the row."""
    y = whole[0]
    stage.set(1, 24000); stage.set_tempo(1, 1000); stage.set_level(1, 1200, -100)
    a = stage.push({1: sig[:5000]})[1]
    assert a.size == 5000 - D
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([1], [sig[5000:12000]], [False], cap=[10])
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([1, 1], [sig[5000:7000], sig[7000:9000]], [False, False])
    assert e.value.status == Q3_INVALID_ARG
    b = stage.push({1: sig[5000:5100]})[1]                 # (fewer new samples than the look-ahead)
    c = stage.push({1: sig[5100:]}, last=(1,))[1]
    np.testing.assert_array_equal(np.concatenate([a, b, c]).view(np.uint32), y.view(np.uint32))
    assert stage.push({1: sig[:0]}, last=(1,))[1].size == 0
    with pytest.raises(_lib.Q3Error):
        stage.push({1: sig[:10]})                          # a flushed row takes no more samples
    for restart in (lambda: stage.reset(1), lambda: stage.set(1, 24000), lambda: stage.set_tempo(1, 1000), lambda: stage.set_level(1, 1200, -100)):
        restart()
        stage.push({1: sig[:3000]})
        restart()                                          # in mid-stream
        got = run_row(stage, 1, sig, 12000)
        np.testing.assert_array_equal(got.view(np.uint32), y.view(np.uint32))
    with pytest.raises(_lib.Q3Error) as e:
        stage.set_level(1, 2401, -100)
    assert e.value.status == Q3_INVALID_ARG
    stage.reset(1)
    got = run_row(stage, 1, sig[:8000], 8000)              # the refused setting changed nothing
    np.testing.assert_array_equal(got[:7000].view(np.uint32), y[:7000].view(np.uint32))
