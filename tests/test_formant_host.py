"""The formant step's host side (no GPU): the warp a row carries, the refusals, the streaming rule, the bound, the
tables — and that the float64 restatement (formant_cases.formant_ref), the reference of the GPU tests, does what the step is for."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
import formant_cases as fc

L = _lib.lib
Q3_INVALID_ARG = 1


@pytest.mark.parametrize("tempo,cents,keep,fcents", [(1000, 400, 1, 0), (1000, -300, 1, 0), (1000, 0, 0, 200), (1000, 400, 1, -200), (800, 200, 1, 0),
                                                      (1250, 600, 1, 600), (1000, 0, 1, 0), (1000, 300, 0, 0), (1250, 0, 0, 0)])
def test_plan(tempo, cents, keep, fcents):
    te = int(round(tempo / 2.0 ** (cents / 1200.0))) if cents else tempo
    want = np.float32((tempo / te if keep else 1.0) / 2.0 ** (fcents / 1200.0))
    omega, runs = api.pcm_stage_formant_plan(tempo, cents, keep, fcents)
    assert omega == want and runs == (want != np.float32(1.0))
    assert runs == (fcents != 0 or (keep == 1 and cents != 0))


@pytest.mark.parametrize("call", [
    lambda: L.q3_pcm_stage_formant_plan(1000, 0, 1, 601, None, None), lambda: L.q3_pcm_stage_formant_plan(1000, 0, 0, -601, None, None),
    lambda: L.q3_pcm_stage_formant_plan(1000, 0, 2, 0, None, None), lambda: L.q3_pcm_stage_formant_plan(1000, 0, -1, 0, None, None),
    lambda: L.q3_pcm_stage_formant_plan(800, 1200, 1, 0, None, None),       # the pitch's own refusal: the stretcher would run at 400
    lambda: L.q3_pcm_stage_set_formant(None, 0, 1, 0), lambda: L.q3_session_set_formant(None, 0, 1, 0), lambda: L.q3_batcher_ticket_formant(None, 1, 1, 0),
    lambda: L.q3_pcm_stage_formant_count(10, 0, None), lambda: L.q3_pcm_stage_bound_formant(24000, 1000, 0, 0, 5, 400, 10, ctypes.byref(ctypes.c_size_t())),
    lambda: L.q3_pcm_stage_formant_tables(ctypes.byref(ctypes.c_float()), 1, None, 0, None, None)])
def test_refusals(call):
    assert call() == Q3_INVALID_ARG


def test_counts():
    out = [api.pcm_stage_formant_count(F) for F in range(3000)]
    assert out == [fc.H * max(0, F // fc.H - 3) for F in range(3000)]
    assert all(b >= a for a, b in zip(out, out[1:])) and all(o <= max(0, F - 768) for F, o in enumerate(out))
    assert out[1023] == 0 and out[1024] == 256
    assert all(api.pcm_stage_formant_count(F, True) == F for F in (0, 1, 1023, 1024, 6000))


def test_bound_over_every_split():
    """A 6000-sample row at 24 kHz with the step alone (what leaves the step leaves the stage), in two pushes cut anywhere."""
    N = 6000
    bound = [api.pcm_stage_bound(24000, n, formant=True) for n in range(N + 1)]
    assert bound == [n + 1023 for n in range(N + 1)]
    for a in range(N + 1):
        first = api.pcm_stage_formant_count(a)
        assert first <= bound[a] and N - first <= bound[N - a]
    # in its place in the chain: behind a pitch step's cap, in front of a level's and a resampler's
    assert api.pcm_stage_bound(16000, 960, 1250, True, 200, (50, 400), True) > api.pcm_stage_bound(16000, 960, 1250, True, 200, (50, 400))
    assert api.pcm_stage_bound(24000, 960, 1000, False, 200, None, True) == api.pcm_stage_bound(24000, 960, 1000, False, 200) + 1023


def test_tables():
    tw, win, N, H = api.pcm_stage_formant_tables()
    assert (N, H) == (fc.N, fc.H) and tw.shape == (N,) and win.shape == (N,)
    want = np.exp(-2j * np.pi * np.arange(N) / N)
    for got, ref in ((tw.real, want.real), (tw.imag, want.imag), (win, fc.window())):
        assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()


def test_reference_keeps_the_formants():
    """+400 cents of varispeed and stretch move the probe's 300-1100 Hz centroid by delta0 (the vowel at f0 p under its envelope
    read at f / p); the reference with keep = 1 brings it back to within a quarter of that. An omega of 1 changes nothing."""
    omega, _ = api.pcm_stage_formant_plan(1000, 400, 1, 0)
    plain, pitched = fc.vowel(), fc.vowel(120.0 * float(omega), float(omega))
    c0 = fc.band_centroid(plain)
    delta0 = fc.band_centroid(pitched) - c0
    delta = fc.band_centroid(fc.formant_ref(pitched, omega)) - c0
    print(f"centroid {c0:.1f} Hz, moved by {delta0:.1f} Hz, with keep by {delta:.1f} Hz")
    assert delta0 > 100.0 and abs(delta) < delta0 / 4.0
    assert np.abs(fc.formant_ref(plain, 1.0) - plain).max() < 1e-12
