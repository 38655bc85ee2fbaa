"""The reference-audio intake, the parts that need no device: its tables against an f64 restatement of q3_resample's
filter, its sample counts against q3_resample's, the G.711 expansion against the ITU-T formulas and tests/golden/g711_tables.npz,
q3_wav_info on files of every format the intake reads, and the refusals of the new entry points."""
import ctypes
import os

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
from intake_cases import FORMATS, LM, RATES, chunk, clip_samples, encode, np_taps, ulp_diff, write_wav

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz")
NEW = ["q3_wav_info", "q3_g711_to_pcm16", "q3_intake_taps", "q3_intake_count", "q3_ref_audio_create_many", "q3_ref_audio_create",
       "q3_ref_audio_from_wav", "q3_ref_audio_info", "q3_ref_audio_read", "q3_ref_audio_free", "q3_spk_encode_ref", "q3_mimi_encode_ref"]


def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.lib.q3_abi_version() == 1
    assert ctypes.sizeof(_lib.CClip) == 32 and ctypes.sizeof(_lib.CWavDesc) == 40
    for n in ("from_wav", "from_samples", "many", "samples", "duration", "close"):
        assert callable(getattr(api.RefAudio, n)), n


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("sr", RATES)
def test_taps_match_numpy_restatement(sr):
    t, L, M = api.intake_taps(sr)
    h, L2, M2 = np_taps(sr)
    assert (L, M) == (L2, M2) == LM[sr] and t.shape == (L, 128) and t.dtype == np.float32
    assert ulp_diff(t, h.astype(np.float32)).max() <= 1


def test_rates_refused():
    for sr in (3999, 96001, 192000, 44101):
        with pytest.raises(_lib.Q3Error) as e:
            api.intake_taps(sr)
        assert e.value.status == 7 and "q3_resample" in str(e.value), sr      # Q3_UNSUPPORTED, and where to go instead
        with pytest.raises(_lib.Q3Error) as e:
            api.intake_count(sr, 100)
        assert e.value.status == 7, sr
    for sr in (12000, 24000, 4000):
        api.intake_taps(sr)
    buf = np.empty(10, np.float32); L = ctypes.c_int(); M = ctypes.c_int()
    assert _lib.lib.q3_intake_taps(8000, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(L), ctypes.byref(M)) == 1     # too small


@pytest.mark.parametrize("sr", RATES + [24000])
def test_counts_are_q3_resamples(sr):
    x = np.zeros(44100, np.float32)
    for n in (1, 63, 64, 65, 1000, 44100):
        no = ctypes.c_int64()
        _lib.check(_lib.lib.q3_resample(x.ctypes.data_as(ctypes.c_void_p), n, sr, 24000, None, 0, ctypes.byref(no)))
        assert api.intake_count(sr, n) == no.value, (sr, n)


# ---------------------------------------------------------------- G.711
def _expand_ulaw(b):
    u = ~b & 0xFF
    t = ((u & 0x0F) << 3) + 0x84
    t <<= (u & 0x70) >> 4
    return 0x84 - t if u & 0x80 else t - 0x84


def _expand_alaw(b):
    a = b ^ 0x55
    t = (a & 0x0F) << 4
    seg = (a & 0x70) >> 4
    if seg == 0:
        t += 8
    elif seg == 1:
        t += 0x108
    else:
        t = (t + 0x108) << (seg - 1)
    return t if a & 0x80 else -t


def test_g711_expansion_all_bytes():
    allb = np.arange(256, dtype=np.uint8)
    np.testing.assert_array_equal(api.g711_expand(allb, "ulaw"), np.array([_expand_ulaw(int(b)) for b in allb], np.int16))
    np.testing.assert_array_equal(api.g711_expand(allb, "alaw"), np.array([_expand_alaw(int(b)) for b in allb], np.int16))
    assert api.g711_expand(np.zeros(0, np.uint8), "ulaw").size == 0
    assert _lib.lib.q3_g711_to_pcm16(None, 4, 2, None) == 1 and _lib.lib.q3_g711_to_pcm16(allb.ctypes.data_as(ctypes.c_void_p), 4, 0, None) == 1
    with pytest.raises(ValueError):
        api.g711_expand(allb, "s16")


def test_g711_round_trip_through_golden_tables():
    """encode(expand(b)) == b, with the encoder read from the committed tables (indexed by v + 32768): every A-law byte, and every
    mu-law byte except 0x7F, which expands to 0 and therefore encodes as 0xFF."""
    z = np.load(GOLDEN)
    tabs = {"ulaw": z["ulaw"], "alaw": z["alaw"]}
    allb = np.arange(256, dtype=np.uint8)
    for law in ("ulaw", "alaw"):
        v = api.g711_expand(allb, law).astype(np.int64)
        back = tabs[law].reshape(-1)[v + 32768].astype(np.uint8)
        keep = allb != 0x7F if law == "ulaw" else np.ones(256, bool)
        np.testing.assert_array_equal(back[keep], allb[keep])
        np.testing.assert_array_equal(api.g711(v.astype(np.int16), law)[keep], allb[keep])      # and through the library's own encoder
    assert api.g711_expand(np.array([0x7F], np.uint8), "ulaw")[0] == 0
    assert tabs["ulaw"].reshape(-1)[32768] == 0xFF


# ---------------------------------------------------------------- q3_wav_info
def _agrees_with_wav_read(path, info):
    a = api.load_wav(path)
    assert (a.samples.size, a.sample_rate) == (info.frames, info.sample_rate), path


def test_wav_info_of_the_library_writers(tmp_path):
    x = (0.2 * np.sin(np.arange(501) * 0.05)).astype(np.float32)
    p = str(tmp_path / "p16.wav"); api.save_wav(p, x, 22050)
    i = api.wav_info(p)
    assert i == api.WavInfo("s16", 1, 16, 22050, 501, 44, 1002)
    _agrees_with_wav_read(p, i)
    for law, rate in (("ulaw", 8000), ("alaw", 16000)):
        p = str(tmp_path / f"{law}.wav"); api.save_wav_g711(p, api.g711(api.pcm16(x), law), rate, law)
        i = api.wav_info(p)
        # 12 RIFF + (8 + 18) fmt + (8 + 4) fact + 8 data header
        assert i == api.WavInfo(law, 1, 8, rate, 501, 58, 501), law
        with pytest.raises(_lib.Q3Error):      # q3_wav_read itself is not changed: it still takes PCM and float alone
            api.load_wav(p)


@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32"])
@pytest.mark.parametrize("ch", [1, 2, 3])
def test_wav_info_by_hand(tmp_path, fmt, ch):
    raw = encode(clip_samples(101, ch, seed=ch), fmt)
    bits = FORMATS[fmt][1]
    p = write_wav(tmp_path / "a.wav", raw, fmt, ch, 44100)
    i = api.wav_info(p)
    assert i == api.WavInfo(fmt, ch, bits, 44100, 101, 44, 101 * ch * bits // 8)
    _agrees_with_wav_read(p, i)
    # an odd-length LIST chunk in front of data: its pad byte counts
    p = write_wav(tmp_path / "b.wav", raw, fmt, ch, 32000, front=chunk(b"LIST", b"INFOabc"))
    i = api.wav_info(p)
    assert (i.fmt, i.frames, i.data_offset, i.sample_rate) == (fmt, 101, 44 + 8 + 8, 32000)
    assert open(p, "rb").read()[i.data_offset:i.data_offset + i.data_bytes] == raw
    _agrees_with_wav_read(p, i)
    # WAVE_FORMAT_EXTENSIBLE
    p = write_wav(tmp_path / "c.wav", raw, fmt, ch, 48000, extensible=True)
    i = api.wav_info(p)
    assert (i.fmt, i.channels, i.bits, i.frames, i.data_offset) == (fmt, ch, bits, 101, 12 + 8 + 40 + 8)
    _agrees_with_wav_read(p, i)


def test_wav_info_refusals(tmp_path):
    L = _lib.lib; d = _lib.CWavDesc()
    assert L.q3_wav_info(None, ctypes.byref(d)) == 1 and L.q3_wav_info(b"/nonexistent.wav", None) == 1
    assert L.q3_wav_info(b"/nonexistent.wav", ctypes.byref(d)) == 2 and L.q3_last_error()
    p = tmp_path / "x.wav"; p.write_bytes(b"RIFF\0\0\0\0WAVX")
    assert L.q3_wav_info(str(p).encode(), ctypes.byref(d)) == 2
    p2 = write_wav(tmp_path / "y.wav", b"\0" * 16, "s16", 1, 8000)
    raw = bytearray(open(p2, "rb").read()); raw[34] = 12      # 12-bit PCM
    open(p2, "wb").write(bytes(raw))
    assert L.q3_wav_info(p2.encode(), ctypes.byref(d)) == 7


# ---------------------------------------------------------------- refusals of the device entry points, before any device call
def test_refusals_need_no_device():
    L = _lib.lib
    h = ctypes.c_void_p(); n = ctypes.c_int64(); i = ctypes.c_int()
    data = np.zeros(64, np.int16)

    def clip(frames=16, channels=1, rate=16000, fmt=1, ptr=True):
        c = _lib.CClip(); c.data = data.ctypes.data if ptr else None
        c.frames, c.channels, c.sample_rate, c.format = frames, channels, rate, fmt
        return c
    three = (_lib.CClip * 3)(clip(), clip(), clip(rate=44101))
    hs = (ctypes.c_void_p * 3)()
    calls = [
        (lambda: L.q3_ref_audio_create(0, None, ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip()), None), 1),
        (lambda: L.q3_ref_audio_create(-1, ctypes.byref(clip()), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(frames=0)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(channels=0)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(channels=9)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(fmt=7)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(fmt=-1)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(ptr=False)), ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(rate=44101)), ctypes.byref(h)), 7),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(rate=192000)), ctypes.byref(h)), 7),
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(frames=1, rate=96000)), ctypes.byref(h)), 1),      # n_out 0
        (lambda: L.q3_ref_audio_create(0, ctypes.byref(clip(frames=24000 * 121, rate=24000)), ctypes.byref(h)), 1),      # longer than 120 s
        (lambda: L.q3_ref_audio_create_many(0, 0, three, hs), 1),
        (lambda: L.q3_ref_audio_create_many(0, 65, three, hs), 1),
        (lambda: L.q3_ref_audio_create_many(0, 3, None, hs), 1),
        (lambda: L.q3_ref_audio_create_many(0, 3, three, None), 1),
        (lambda: L.q3_ref_audio_create_many(0, 3, three, hs), 7),
        (lambda: L.q3_ref_audio_from_wav(None, 0, ctypes.byref(h)), 1),
        (lambda: L.q3_ref_audio_from_wav(b"/nonexistent.wav", 0, None), 1),
        (lambda: L.q3_ref_audio_from_wav(b"/nonexistent.wav", 0, ctypes.byref(h)), 2),
        (lambda: L.q3_ref_audio_info(None, ctypes.byref(n), None, None, None, None), 1),
        (lambda: L.q3_ref_audio_read(None, None, 0, ctypes.byref(n)), 1),
        (lambda: L.q3_spk_encode_ref(None, None, None), 1),
        (lambda: L.q3_mimi_encode_ref(None, None, None, 0, ctypes.byref(i), None), 1),
        (lambda: L.q3_intake_count(16000, -1, ctypes.byref(n)), 1),
        (lambda: L.q3_intake_count(16000, 10, None), 1),
    ]
    for k, (f, want) in enumerate(calls):
        assert f() == want, (k, L.q3_last_error())
        assert L.q3_last_error(), k
    assert not h.value and not any(hs)                       # nothing was created, the handles are untouched
    assert b"q3_resample" in (L.q3_ref_audio_create(0, ctypes.byref(clip(rate=44101)), ctypes.byref(h)), L.q3_last_error())[1]
    L.q3_ref_audio_free(None)                                # free(NULL) is a no-op
    with pytest.raises(ValueError):
        api.RefAudio.from_samples(b"\0\0", 16000, "s12")
