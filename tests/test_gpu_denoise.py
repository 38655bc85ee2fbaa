"""The spectral noise suppressor on the device (k_dn_analysis, k_dn_gain, k_dn_synthesis, k_dn_level) against the
float64 restatement of its definition (denoise_cases.reference), on the gated-tone-plus-noise probe.

The allowance of a sample is 128 * 2^-24 * max|x|: two 512-point f32 transforms, two windows and a four-term overlap-add round on
the order of log2(N) times each, and x -> y is continuous (min, box mean and xi / (1 + xi) have no jumps); a wrong bin, window,
frame offset or scale shows as 1e-3 of the peak or more."""
import functools

import numpy as np
import pytest

from qwen3_tts_rs_amd import api
from denoise_cases import LENGTHS, noise_figures, probe, reference, snr_db

pytestmark = pytest.mark.gpu
LONG = 72000                                                     # the 3 s probe


@functools.lru_cache(maxsize=None)
def _want(n, reduce_db):
    return reference(probe(LONG)[0][:n], reduce_db)


def _ref(n):
    return api.RefAudio.from_samples(probe(LONG)[0][:n], 24000, "f32")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("reduce_db", [0.0, 12.0, 30.0])
@pytest.mark.parametrize("n", LENGTHS)
def test_against_float64(n, reduce_db):
    x = probe(LONG)[0][:n]
    src = _ref(n)
    out = src.denoise(reduce_db)
    y = out.samples()
    assert (len(out), out.source_rate, out.source_format, out.source_channels) == (n, 24000, "f32", 1)
    allow = 128 * 2.0 ** -24 * float(np.abs(x).max())
    share = float(np.abs(y - _want(n, reduce_db)["y"]).max()) / allow
    print(f"n {n}, reduce_db {reduce_db:g}: largest error / allowance = {share:.3f}")
    assert share <= 1.0, (n, reduce_db, share)
    if reduce_db == 0.0 or n <= 384:                             # G = 1: the input comes back
        assert float(np.abs(y - x.astype(np.float64)).max()) <= allow, (n, reduce_db)
    src.close(); out.close()


def test_effect_is_the_references():
    noisy, clean = probe(LONG)
    want = _want(LONG, 12.0)["y"]
    assert snr_db(want, clean) - snr_db(noisy, clean) >= 6.0     # the algorithm itself
    src = _ref(LONG)
    out = src.denoise(12.0)
    got = snr_db(out.samples(), clean)
    print(f"SNR in {snr_db(noisy, clean):.2f} dB, float64 {snr_db(want, clean):.2f} dB, device {got:.2f} dB")
    assert abs(got - snr_db(want, clean)) <= 0.05
    src.close(); out.close()


def test_batch_is_solo_bit_for_bit():
    refs = [_ref(n) for n in (25111, 513, 24000)]
    before = [r.samples() for r in refs]
    many = api.RefAudio.denoise_many(refs, [12.0, 30.0, 6.0])
    for r, m, db, b in zip(refs, many, (12.0, 30.0, 6.0), before):
        one = r.denoise(db)
        np.testing.assert_array_equal(_bits(m.samples()), _bits(one.samples()))
        np.testing.assert_array_equal(_bits(r.samples()), _bits(b))      # the inputs are untouched
        one.close(); m.close(); r.close()


def test_layers_and_noise_estimate():
    import qwen3_tts_rs_amd as q
    src = _ref(LONG)
    nz, snr = src.noise()
    want = noise_figures(_want(LONG, 12.0))
    print(f"noise {nz:.2f} dBFS (float64 {want[0]:.2f}), SNR {snr:.2f} dB (float64 {want[1]:.2f})")
    assert abs(nz - want[0]) <= 0.1 and abs(snr - want[1]) <= 0.1
    out = src.denoise()
    y = out.samples()
    spk = q.SpeakerEncoder.from_synthetic(q.tiny_speaker_config(64))
    np.testing.assert_array_equal(_bits(spk.encode_ref(out)), _bits(spk.encode(y, 24000)))
    mimi = q.SpeechEncoder.from_synthetic(q.tiny_speech_config())
    np.testing.assert_array_equal(mimi.encode_ref(out), mimi.encode(y, 24000))
    spk.close(); mimi.close(); src.close(); out.close()
    with pytest.raises(api._lib.Q3Error) as e:                   # too short for a floor
        _ref(384).noise()
    assert e.value.status == 7
