"""Many reference clips in one packed pass of each voice-clone encoder: for every clip of a many-clip call the codes,
the three speech-encoder taps, the speaker embedding and the six speaker taps are BIT-equal to that clip's own encode_ref,
whatever the other clips are and wherever its slot lies. Each clip's single-clip result is computed once per module."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api

pytestmark = pytest.mark.gpu
SEED = 1234
FILL = np.float32("nan")        # no finite result equals it, and an unwritten element shows


def make_ref(n, seed):
    """n samples at 24 kHz f32: the intake hands them on bit for bit."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 24000.0
    x = (0.3 * np.sin(2 * np.pi * (110.0 + 7.0 * seed) * t + seed) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return api.RefAudio.from_samples(x, 24000, "f32")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- speech encoder
def mimi_alone(enc, ref):
    taps = [np.full(s, FILL, np.float32) for s in enc.tap_shapes(ref.n_samples)]
    codes = enc.encode_ref(ref, taps=taps)
    assert not any(np.isnan(t).any() for t in taps)           # every tap was written
    return codes, taps


def mimi_check(enc, refs, alone):
    """one encode_refs over `refs`; `alone`: each clip's own (codes, taps)"""
    taps = [[np.full(s, FILL, np.float32) for s in enc.tap_shapes(r.n_samples)] for r in refs]
    codes = enc.encode_refs(refs, taps=taps)
    assert len(codes) == len(refs)
    for i, (r, (c1, t1)) in enumerate(zip(refs, alone)):
        assert codes[i].shape == (enc.frames(r.n_samples), enc.config.n_q), i
        np.testing.assert_array_equal(codes[i], c1, err_msg=f"codes of clip {i} ({r.n_samples} samples)")
        for k in range(3):
            np.testing.assert_array_equal(bits(taps[i][k]), bits(t1[k]), err_msg=f"tap {k} of clip {i} ({r.n_samples} samples)")


TINY_LENGTHS = [1, 95, 96, 97, 480, 2000, 5003]


@pytest.fixture(scope="module")
def tiny_mimi():
    enc = q.SpeechEncoder.from_synthetic(q.tiny_speech_config(), seed=SEED)
    assert enc.pack_plan(TINY_LENGTHS).packable
    refs = [make_ref(n, 10 + i) for i, n in enumerate(TINY_LENGTHS)]
    alone = [mimi_alone(enc, r) for r in refs]
    yield enc, refs, alone
    for r in refs:
        r.close()
    enc.close()


def test_tiny_mimi_many_clips(tiny_mimi):
    enc, refs, alone = tiny_mimi
    assert enc.pack_plan(TINY_LENGTHS).n_passes == 1
    mimi_check(enc, refs, alone)


def test_tiny_mimi_reversed(tiny_mimi):
    enc, refs, alone = tiny_mimi
    mimi_check(enc, refs[::-1], alone[::-1])


def test_tiny_mimi_one_clip(tiny_mimi):
    enc, refs, alone = tiny_mimi
    for i in (0, 3, 6):
        mimi_check(enc, [refs[i]], [alone[i]])


def test_tiny_mimi_same_clip_twice(tiny_mimi):
    enc, refs, alone = tiny_mimi
    i = TINY_LENGTHS.index(2000)
    mimi_check(enc, [refs[i], refs[2], refs[i]], [alone[i], alone[2], alone[i]])


def test_tiny_mimi_codes_only_and_lengths(tiny_mimi):
    enc, refs, alone = tiny_mimi
    codes = enc.encode_refs(refs[:3])                       # no taps
    for c, (c1, _) in zip(codes, alone):
        np.testing.assert_array_equal(c, c1)
    hs = (ctypes.c_void_p * 3)(*[r._h.value for r in refs[4:7]]); nf = (ctypes.c_int * 3)()
    _lib.check(_lib.lib.q3_mimi_encode_refs(enc._h, hs, 3, None, 0, nf, None))
    assert list(nf) == [enc.frames(n) for n in TINY_LENGTHS[4:7]]
    buf = np.full((sum(nf) - 1, enc.config.n_q), 0xABCD, np.uint32)      # one frame short: refused, nothing written
    assert _lib.lib.q3_mimi_encode_refs(enc._h, hs, 3, buf.ctypes.data_as(ctypes.c_void_p), buf.shape[0], nf, None) == 1
    assert b"too small" in _lib.lib.q3_last_error() and (buf == 0xABCD).all()


def test_tiny_mimi_two_passes(tiny_mimi):
    """two 70 s clips: their slots exceed one pass's 120 s, so the call runs two passes"""
    enc = tiny_mimi[0]
    n = 24000 * 70
    assert enc.pack_plan([n, n]).passes == [0, 1]
    refs = [make_ref(n, 31), make_ref(n, 32)]
    mimi_check(enc, refs, [mimi_alone(enc, r) for r in refs])
    for r in refs:
        r.close()


def test_production_mimi():
    """0.31 s, 2.0 s and 10.6 s: the last has more than 250 columns at 25 Hz, so the attention window's cut lies inside a packed clip"""
    enc = q.SpeechEncoder.from_synthetic(None, seed=SEED)
    lengths = [7440, 48000, 254400]
    assert enc.tap_shapes(lengths[2])[0][1] > enc.config.window
    refs = [make_ref(n, 40 + i) for i, n in enumerate(lengths)]
    mimi_check(enc, refs, [mimi_alone(enc, r) for r in refs])
    for r in refs:
        r.close()
    enc.close()


# ---------------------------------------------------------------- speaker encoder
def spk_alone(enc, ref):
    T = enc.mel_frames(ref.n_samples)
    taps = [np.full(s, FILL, np.float32) for s in enc.tap_shapes(T)]
    emb = enc.encode_ref(ref)
    fwd = enc.forward(enc.mel(ref.samples()), taps=taps)     # the taps of the same kernels on the same mel
    np.testing.assert_array_equal(bits(fwd), bits(emb))
    assert not any(np.isnan(t).any() for t in taps)           # every tap was written
    return emb, taps


def spk_check(enc, refs, alone):
    taps = [[np.full(s, FILL, np.float32) for s in enc.tap_shapes(enc.mel_frames(r.n_samples))] for r in refs]
    embs = enc.encode_refs(refs, taps=taps)
    assert embs.shape == (len(refs), enc.config.enc_dim)
    for i, (r, (e1, t1)) in enumerate(zip(refs, alone)):
        for k in range(6):
            np.testing.assert_array_equal(bits(taps[i][k]), bits(t1[k]), err_msg=f"tap {k} of clip {i} ({r.n_samples} samples)")
        np.testing.assert_array_equal(bits(embs[i]), bits(e1), err_msg=f"embedding of clip {i} ({r.n_samples} samples)")
    np.testing.assert_array_equal(bits(enc.encode_refs(refs)), bits(embs))      # without taps


def smallest_speaker_clip():
    """the first length whose mel frames outnumber the widest reflect padding (4 columns at the default kernel sizes and dilations)"""
    n = 1
    while q.SpeakerEncoder.mel_frames(n) <= 4:
        n += 1
    return n


@pytest.mark.parametrize("name,cfg,lengths", [
    ("tiny", q.tiny_speaker_config, [5000, 48123, 30000, smallest_speaker_clip()]),
    ("full", q.SpeakerEncoderConfig, [31200, 96000, 12000])])
def test_speaker_many_clips(name, cfg, lengths):
    enc = q.SpeakerEncoder.from_synthetic(cfg(), seed=SEED)
    refs = [make_ref(n, 50 + i) for i, n in enumerate(lengths)]
    alone = [spk_alone(enc, r) for r in refs]
    spk_check(enc, refs, alone)
    spk_check(enc, refs[::-1], alone[::-1])
    spk_check(enc, [refs[1]], [alone[1]])
    for r in refs:
        r.close()
    enc.close()


def test_all_or_nothing():
    """a clip too short for the reflect padding, and a null entry: a status with the clip's index, and the output keeps its fill"""
    enc = q.SpeakerEncoder.from_synthetic(q.tiny_speaker_config(), seed=SEED)
    mimi = q.SpeechEncoder.from_synthetic(q.tiny_speech_config(), seed=SEED)
    short = smallest_speaker_clip() - 1
    refs = [make_ref(5000, 60), make_ref(6000, 61), make_ref(short, 62), make_ref(7000, 63)]
    with pytest.raises(_lib.Q3Error, match=r"clip 2: reference audio too short") as e:
        enc.encode_refs(refs)
    assert e.value.status == 1
    hs = (ctypes.c_void_p * 4)(*[r._h.value for r in refs])
    out = np.full((4, enc.config.enc_dim), FILL, np.float32)
    assert _lib.lib.q3_spk_encode_refs(enc._h, hs, 4, out.ctypes.data_as(ctypes.c_void_p), None) == 1
    assert b"clip 2" in _lib.lib.q3_last_error() and np.isnan(out).all()
    hs[1] = None
    assert _lib.lib.q3_spk_encode_refs(enc._h, hs, 4, out.ctypes.data_as(ctypes.c_void_p), None) == 1
    assert b"clip 1: null entry" in _lib.lib.q3_last_error() and np.isnan(out).all()
    nf = (ctypes.c_int * 4)(-5, -5, -5, -5)
    assert _lib.lib.q3_mimi_encode_refs(mimi._h, hs, 4, None, 0, nf, None) == 1
    assert b"clip 1: null entry" in _lib.lib.q3_last_error() and list(nf) == [-5] * 4
    # an encoder on no device: every clip lies on another one
    off = q.SpeakerEncoder(q.tiny_speaker_config(), device=-1)
    hs[1] = refs[1]._h.value
    assert _lib.lib.q3_spk_encode_refs(off._h, hs, 4, out.ctypes.data_as(ctypes.c_void_p), None) == 1
    assert b"clip 0: reference audio is on device" in _lib.lib.q3_last_error() and np.isnan(out).all()
    # the speech encoder takes any length from one sample: the same list is fine there
    codes = mimi.encode_refs(refs)
    for c, r in zip(codes, refs):
        np.testing.assert_array_equal(c, mimi.encode_ref(r))
    for r in refs:
        r.close()
    off.close(); enc.close(); mimi.close()
