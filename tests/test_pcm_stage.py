"""The output stage (DESIGN 4.12, q3_pcm_stage_*): 24 kHz f32 -> a requested rate, f32 or PCM16, with state per row. Host-only
parts (rates, taps, bound) run anywhere; the `gpu` tests feed random PCM — no model — and compare bitwise with one-shot runs of
the same stage, and against the host resampler q3_resample within the rounding bound of the f32 dot product."""
import ctypes
import math

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import manifest_handle

NEW = ["q3_pcm_stage_create", "q3_pcm_stage_free", "q3_pcm_stage_set", "q3_pcm_stage_reset", "q3_pcm_stage_push", "q3_pcm_stage_bound",
       "q3_pcm_stage_taps", "q3_codec_stream_push_out", "q3_session_set_output", "q3_session_next_chunks_out", "q3_batcher_ticket_output",
       "q3_batcher_read_out"]
RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000]


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.lib.q3_abi_version() == 1
    assert callable(api.Qwen3TTS.pcm_stage) and callable(api.Session.set_output) and callable(api.Session.next_chunks_out)
    assert callable(api.resample_gpu) and callable(api.Batcher.ticket_output)
    for n in ("set", "reset", "push", "close"):
        assert callable(getattr(api.PcmStage, n)), n


def test_no_device_no_fallback():
    """Null handles and a manifest-only model: a status and a message, nothing routed elsewhere (the pattern of
    test_codec_stream.py::test_no_device_no_fallback)."""
    L = _lib.lib
    ps = ctypes.c_void_p(); i = ctypes.c_int(); sz = ctypes.c_size_t()
    assert L.q3_pcm_stage_create(-1, 2, 1920, ctypes.byref(ps)) != 0      # the device of a manifest-only model
    assert b"device" in L.q3_last_error() and not ps.value
    h = manifest_handle(q.tiny())
    gm = api.Qwen3TTS(q.tiny(), device=-1, _handle=h)
    with pytest.raises(_lib.Q3Error):
        gm.pcm_stage(2, 1920)
    calls = [
        lambda: L.q3_pcm_stage_create(0, 0, 1920, ctypes.byref(ps)),
        lambda: L.q3_pcm_stage_create(0, 1, 1920, None),
        lambda: L.q3_pcm_stage_set(None, 0, 16000, 1),
        lambda: L.q3_pcm_stage_reset(None, 0),
        lambda: L.q3_pcm_stage_push(None, 0, None, None, None, None, None, None, None),
        lambda: L.q3_pcm_stage_bound(16000, 10, None),
        lambda: L.q3_codec_stream_push_out(None, 0, None, None, None, None, None, None, None, None, None),
        lambda: L.q3_session_set_output(None, 16000, 1),
        lambda: L.q3_session_next_chunks_out(None, None, None, ctypes.byref(sz), ctypes.byref(i)),
        lambda: L.q3_batcher_ticket_output(None, 1, 16000, 1),
        lambda: L.q3_batcher_read_out(None, 1, None, 0, ctypes.byref(sz), ctypes.byref(i)),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error(), k
    L.q3_pcm_stage_free(None)      # free(NULL) is a no-op
    gm.close()


def test_rates():
    for sr in RATES + [12000, 24000, 96000, 4000]:
        _, L, M = api.pcm_stage_taps(sr)
        g = math.gcd(sr, 24000)
        assert (L, M) == (sr // g, 24000 // g), sr
    for sr in (47999, 3000, 0, 96001, 192000):
        with pytest.raises(_lib.Q3Error) as e:
            api.pcm_stage_taps(sr)
        assert e.value.status == 7, sr                    # Q3_UNSUPPORTED
        with pytest.raises(_lib.Q3Error) as e:
            api.pcm_stage_bound(sr, 10)
        assert e.value.status == 7, sr


def np_taps(sr):
    """The window-sinc of q3_resample (q3_io.cpp) at t - c = p / L, in f64: row p = weights of inputs c - 63 .. c + 64."""
    g = math.gcd(sr, 24000); L, M = sr // g, 24000 // g
    ratio = L / M
    fc = 0.95 * min(ratio, 1.0)
    p = np.arange(L, dtype=np.float64)[:, None]; j = np.arange(128, dtype=np.float64)[None, :]
    u = p / L - (j - 63.0)
    v = u / 64.0
    w = 0.35875 + 0.48829 * np.cos(np.pi * v) + 0.14128 * np.cos(2.0 * np.pi * v) + 0.01168 * np.cos(3.0 * np.pi * v)
    xs = np.pi * fc * u
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(np.abs(xs) < 1e-12, 1.0, np.sin(xs) / xs)
    h = fc * sinc * w * w
    h[(v <= -1.0) | (v >= 1.0)] = 0.0
    return h, L, M


def ulp_diff(a, b):
    ia = a.view(np.int32).astype(np.int64); ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("sr", RATES)
def test_taps_match_numpy_restatement(sr):
    t, L, M = api.pcm_stage_taps(sr)
    h, L2, M2 = np_taps(sr)
    assert (L, M) == (L2, M2) and t.shape == (L, 128) and t.dtype == np.float32
    assert ulp_diff(t, h.astype(np.float32)).max() <= 1


def n_emitted(sr, n_in, ended):
    """The streaming rule: outputs i with floor(i M / L) + 64 <= n_in - 1; after the end llround(n_in sr / 24000)."""
    g = math.gcd(sr, 24000); L, M = sr // g, 24000 // g
    if sr == 24000:
        return n_in
    if ended:
        return int(math.floor(n_in * (sr / 24000.0) + 0.5))
    i = 0 if n_in <= 64 else -((-(n_in - 64) * L) // M)
    assert i == 0 or ((i - 1) * M) // L + 64 <= n_in - 1 < (i * M) // L + 64
    return i


@pytest.mark.parametrize("sr", RATES + [24000])
def test_bound_covers_every_split(sr):
    """q3_pcm_stage_bound(sr, n) >= what a push of n samples can return, wherever it falls in a row's stream and with or
    without `last`: before n0 samples (every n0 that matters: the hold-back is 64 samples and the phase repeats every M)."""
    g = math.gcd(sr, 24000); M = 24000 // g
    for n in (1, 64, 65, 1920, 19200):
        bound = api.pcm_stage_bound(sr, n)
        worst = 0
        for n0 in list(range(0, 130 + 2 * M)) + [1920, 19200, 100000]:
            before = n_emitted(sr, n0, False)
            worst = max(worst, n_emitted(sr, n0 + n, False) - before, n_emitted(sr, n0 + n, True) - before)
        assert bound >= worst, (sr, n, bound, worst)
        assert bound <= worst + 2, (sr, n, bound, worst)      # ... and is not a loose one


# ---------------------------------------------------------------- GPU, random PCM, no model
N = 12000
CUTS = [1, 63, 64, 65, 127, 128, 129, 1920, 5000]      # ... and the rest


@pytest.fixture(scope="module")
def pcm():
    return (0.5 * np.random.default_rng(7).standard_normal(N)).astype(np.float32)


@pytest.fixture(scope="module")
def oneshot(pcm):
    """One-shot stage output per (rate, pcm16, scale), computed once and shared."""
    cache = {}

    def get(sr, s16=False, scale=1.0):
        key = (sr, s16, scale)
        if key not in cache:
            ps = api.PcmStage(0, 1, N)
            ps.set(0, sr, s16)
            cache[key] = ps.push({0: pcm * np.float32(scale)}, last=(0,))[0]
            ps.close()
        return cache[key]
    return get


def pieces(x, cuts=CUTS):
    at, out = 0, []
    for c in cuts:
        out.append(x[at:at + c]); at += c
    out.append(x[at:])
    assert at < x.size
    return out


def host_resample(x, sr):
    return api.resample(api.AudioBuffer(x, 24000), sr).samples


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [8000, 16000, 44100, 48000])
def test_chunk_invariance_bitwise(pcm, oneshot, sr):
    """Cut at the edges of the 64-sample hold-back, of the 127 / 128-sample tail and of a frame: the same bits as one push."""
    ps = api.PcmStage(0, 1, N)
    ps.set(0, sr)
    parts = pieces(pcm)
    got, n_in = [], 0
    for k, part in enumerate(parts):
        out = ps.push({0: part}, last=(0,) if k == len(parts) - 1 else ())[0]
        n_in += part.size
        got.append(out)
        assert sum(o.size for o in got) == n_emitted(sr, n_in, k == len(parts) - 1), (k, n_in)      # the streaming rule
    ps.close()
    got = np.concatenate(got)
    assert got.dtype == np.float32
    assert got.size == host_resample(pcm, sr).size                       # q3_resample's n_out
    np.testing.assert_array_equal(got, oneshot(sr))


@pytest.mark.gpu
@pytest.mark.parametrize("sr", RATES)
def test_against_host_resampler(pcm, oneshot, sr):
    """|gpu - host| <= 132 * 2^-24 * sum_j |h[p][j]| |x[c - 63 + j]| for every output sample: one rounding per tap, 128 products,
    127 additions and the host's final cast; holds for any summation order."""
    got = oneshot(sr)
    ref = host_resample(pcm, sr)
    assert got.shape == ref.shape
    h, L, M = np_taps(sr)
    i = np.arange(got.size, dtype=np.int64)
    c, p = (i * M) // L, (i * M) % L
    xpad = np.concatenate([np.zeros(64), np.abs(pcm.astype(np.float64)), np.zeros(64 + 64)])
    idx = (c - 63 + 64)[:, None] + np.arange(128)[None, :]
    mag = (np.abs(h)[p] * xpad[idx]).sum(axis=1)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = 132.0 * 2.0 ** -24 * mag
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"sr {sr}: largest error / bound = {worst:.3f}")
    assert (err <= bound).all(), (sr, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [16000, 24000, 44100])
def test_s16_is_pcm16_of_the_f32_stream(pcm, oneshot, sr):
    scale = 0.78                                        # 0.39 sigma: about 1 % of the samples beyond +-1
    f = oneshot(sr, False, scale); s = oneshot(sr, True, scale)
    assert s.dtype == np.int16 and f.dtype == np.float32
    clipped = float((np.abs(pcm * np.float32(scale)) > 1.0).mean())
    assert 0.003 < clipped < 0.03, clipped
    np.testing.assert_array_equal(s, api.pcm16(f))
    assert (np.abs(s.astype(np.int32)) == 32767).any()


@pytest.mark.gpu
def test_nan_and_clamp_to_s16():
    x = np.array([np.nan, 2.0, -2.0, 0.5, -0.5, 1.0, -1.0, 0.99999, np.inf, -np.inf], np.float32)
    ps = api.PcmStage(0, 1, 64)
    ps.set(0, 24000, True)
    np.testing.assert_array_equal(ps.push({0: x})[0], api.pcm16(x))
    ps.close()


ROWS = {0: (8000, True), 1: (44100, False), 2: (48000, True)}
# {row: samples in this push}; row 1 is absent from pushes 1 and 3, row 0 from push 4; the last push ends every row
ROW_PUSHES = [{0: 100, 1: 1920, 2: 63}, {0: 1920, 2: 1}, {0: 65, 1: 130, 2: 3000}, {0: 700, 2: 1920}, {1: 4000, 2: 64}, {0: 3000, 1: 2000, 2: 1000}]


@pytest.mark.gpu
def test_rows_are_independent(pcm):
    ps = api.PcmStage(0, 3, 4000)
    for r, (sr, s16) in ROWS.items():
        ps.set(r, sr, s16)
    xs = {r: np.roll(pcm, 1000 * r) for r in ROWS}
    at = {r: 0 for r in ROWS}; got = {r: [] for r in ROWS}
    for k, call in enumerate(ROW_PUSHES):
        last = tuple(call) if k == len(ROW_PUSHES) - 1 else ()
        out = ps.push({r: xs[r][at[r]:at[r] + n] for r, n in call.items()}, last=last)
        for r, n in call.items():
            got[r].append(out[r]); at[r] += n
    ps.close()
    for r, (sr, s16) in ROWS.items():
        one = api.PcmStage(0, 1, N)
        one.set(0, sr, s16)
        ref = one.push({0: xs[r][:at[r]]}, last=(0,))[0]
        one.close()
        g = np.concatenate(got[r])
        assert g.dtype == (np.int16 if s16 else np.float32)
        np.testing.assert_array_equal(g, ref)


@pytest.mark.gpu
def test_24k_f32_is_a_copy(pcm):
    ps = api.PcmStage(0, 1, N)                        # a row's default: 24 kHz f32
    at = 0
    for part in pieces(pcm):
        out = ps.push({0: part})[0]
        assert out.dtype == np.float32
        np.testing.assert_array_equal(out.view(np.uint32), part.view(np.uint32))      # nothing held back, the bits
        at += part.size
    assert ps.push({0: pcm[:0]}, last=(0,))[0].size == 0                              # and nothing left to flush
    ps.close()
    np.testing.assert_array_equal(api.resample_gpu(pcm, 24000).samples, pcm)


@pytest.mark.gpu
def test_reset_set_and_refused_pushes(pcm, oneshot):
    sr = 16000
    ps = api.PcmStage(0, 2, N)
    ps.set(0, sr); ps.set(1, sr)
    a, b, c = pcm[:1000], pcm[1000:3000], pcm[3000:]
    first = ps.push({0: a, 1: a})
    # refused: cap too small, a row listed twice, a row out of range, more than max_push_samples — no row moves
    for bad in (lambda: ps._push_lists([0, 1], [b, b], [False, False], cap=[10, 4000]),
                lambda: ps._push_lists([0, 0], [b, b], [False, False]),
                lambda: ps._push_lists([0, 2], [b, b], [False, False]),
                lambda: ps._push_lists([0], [np.zeros(N + 1, np.float32)], [False])):
        with pytest.raises(_lib.Q3Error) as e:
            bad()
        assert e.value.status == 1
    rest = [ps.push({0: b}), ps.push({0: c}, last=(0,))]
    np.testing.assert_array_equal(np.concatenate([first[0]] + [r[0] for r in rest]), oneshot(sr))
    # a flushed row takes no more samples until it is restarted; a second flush returns nothing
    assert ps.push({0: pcm[:0]}, last=(0,))[0].size == 0
    with pytest.raises(_lib.Q3Error):
        ps.push({0: a})
    # reset restarts a row (same rate and format), set restarts it with another
    ps.reset(0)
    np.testing.assert_array_equal(ps.push({0: pcm}, last=(0,))[0], oneshot(sr))
    ps.reset(1)                                          # row 1 was mid-stream
    np.testing.assert_array_equal(ps.push({1: pcm}, last=(1,))[1], oneshot(sr))
    ps.set(1, 48000, True)
    np.testing.assert_array_equal(ps.push({1: pcm}, last=(1,))[1], oneshot(48000, True))
    with pytest.raises(_lib.Q3Error) as e:
        ps.set(1, 47999)
    assert e.value.status == 7
    ps.close()


@pytest.mark.gpu
def test_resample_gpu_one_shot(pcm, oneshot):
    out = api.resample_gpu(api.AudioBuffer(pcm), 16000, pcm16=True)
    assert out.sample_rate == 16000 and out.samples.dtype == np.int16
    np.testing.assert_array_equal(out.samples, oneshot(16000, True))


def test_bound_refuses_above_2_48():
    """q3_pcm_stage_bound follows its siblings' rule: n_in above 2^48 is Q3_INVALID_ARG with a message (it used to multiply on,
    into a signed overflow at 2^62); at and below 2^48 the value is the closed form, unchanged, and the siblings still answer
    for 2^48 although their chains hand the resampler more than that."""
    L = _lib.lib
    n = ctypes.c_size_t()
    for sr, (l, m) in {44100: (147, 80), 8000: (1, 3), 96000: (4, 1), 22050: (147, 160)}.items():
        for n_in in (0, 1, 1920, (1 << 48) - 1, 1 << 48):
            assert L.q3_pcm_stage_bound(sr, n_in, ctypes.byref(n)) == 0
            assert n.value == ((n_in + 64) * l + m - 1) // m + 1, (sr, n_in)
    assert L.q3_pcm_stage_bound(24000, 1 << 48, ctypes.byref(n)) == 0 and n.value == 1 << 48
    for sr in (24000, 44100):
        for n_in in ((1 << 48) + 1, 1 << 62, (1 << 63) - 1, (1 << 64) - 1):
            n.value = 7
            assert L.q3_pcm_stage_bound(sr, n_in, ctypes.byref(n)) == 1 and b"above 2^48" in L.q3_last_error(), (sr, n_in)
            assert n.value == 7
    for f in (lambda: L.q3_pcm_stage_bound_tempo(44100, 500, 1 << 48, ctypes.byref(n)),
              lambda: L.q3_pcm_stage_bound_level(44100, 500, 1 << 48, ctypes.byref(n)),
              lambda: L.q3_pcm_stage_bound_pitch(44100, 1000, 1200, 1, 1 << 48, ctypes.byref(n))):
        n.value = 0
        assert f() == 0 and n.value > (1 << 48), L.q3_last_error()
    assert L.q3_pcm_stage_bound_tempo(44100, 500, 1 << 48, ctypes.byref(n)) == 0 and n.value > 2 * (1 << 48)
    assert L.q3_pcm_stage_bound_tempo(44100, 500, (1 << 48) + 1, ctypes.byref(n)) == 1
