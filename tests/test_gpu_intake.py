"""The reference-audio intake on the device (k_intake): decode and downmix bit for bit against q3_wav_read at 24 kHz,
the resampler against the host's q3_resample within the rounding bound of the f32 dot product, tiles and edges, and clips of one
launch against the same clips alone. Random PCM, no model."""
import ctypes

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
from intake_cases import RATES, chunk, clip_samples, encode, error_ratio, write_wav

pytestmark = pytest.mark.gpu


def _ref_of(path):
    r = api.RefAudio.from_wav(str(path))
    x = r.samples()
    assert len(r) == x.size and r.sample_rate == 24000 and abs(r.duration() - x.size / 24000.0) < 1e-12
    r.close()
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- decode and downmix, bitwise
@pytest.mark.parametrize("fmt", ["u8", "s16", "s24", "s32", "f32"])
@pytest.mark.parametrize("ch", [1, 2, 3, 8])
def test_decode_is_wav_reads(tmp_path, fmt, ch):
    p = write_wav(tmp_path / "a.wav", encode(clip_samples(777, ch, seed=11 * ch), fmt), fmt, ch, 24000)
    r = api.RefAudio.from_wav(p)
    assert (r.source_rate, r.source_format, r.source_channels, len(r)) == (24000, fmt, ch, 777)
    np.testing.assert_array_equal(_bits(r.samples()), _bits(api.load_wav(p).samples))
    r.close()


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_decode_g711(tmp_path, law):
    raw = encode(clip_samples(777, 1, seed=5), law)
    p = str(tmp_path / "g.wav")
    api.save_wav_g711(p, np.frombuffer(raw, np.uint8), 24000, law)
    want = api.g711_expand(np.frombuffer(raw, np.uint8), law).astype(np.float32) / np.float32(32768.0)
    np.testing.assert_array_equal(_bits(_ref_of(p)), _bits(want))
    allb = np.arange(256, dtype=np.uint8)                    # every byte of the law
    r = api.RefAudio.from_samples(allb, 24000, law)
    np.testing.assert_array_equal(_bits(r.samples()), _bits(api.g711_expand(allb, law).astype(np.float32) / np.float32(32768.0)))
    r.close()


def test_decode_s24_three_channels_off_alignment(tmp_path):
    """The data chunk where a chunk in front puts it. RIFF pads every chunk to an even length — q3_wav_read's walk and q3_wav_info's
    rely on it — so within a file the data starts at an even offset at best: here at 2 mod 4, off every dword. The odd address
    itself comes through from_samples, from a buffer that starts one byte into an allocation."""
    raw = encode(clip_samples(777, 3, seed=9), "s24")
    p = write_wav(tmp_path / "odd.wav", raw, "s24", 3, 24000, front=chunk(b"LIST", b"INFOab"))
    assert api.wav_info(p).data_offset % 4 == 2
    want = api.load_wav(p).samples
    np.testing.assert_array_equal(_bits(_ref_of(p)), _bits(want))
    for shift in (1, 2, 3):
        buf = np.zeros(len(raw) + 8, np.uint8)
        base = (-buf.ctypes.data) % 4 + shift                # an address that is `shift` mod 4
        buf[base:base + len(raw)] = np.frombuffer(raw, np.uint8)
        view = buf[base:base + len(raw)]
        assert view.ctypes.data % 4 == shift
        r = api.RefAudio.from_samples(view, 24000, "s24", 3)
        np.testing.assert_array_equal(_bits(r.samples()), _bits(want), err_msg=str(shift))
        r.close()


# ---------------------------------------------------------------- the resampler against the host
@pytest.mark.parametrize("sr", RATES)
def test_against_host_resampler(tmp_path, sr):
    """|gpu - host| <= 132 * 2^-24 * sum_j |h[p][j]| |x[c - 63 + j]| for every output sample (intake_cases.error_ratio)."""
    rng = np.random.default_rng(sr)
    p = write_wav(tmp_path / "n.wav", encode(0.3 * rng.standard_normal((3000, 1)), "s16"), "s16", 1, sr)
    worst = error_ratio(_ref_of(p), p)
    print(f"sr {sr}: largest error / bound = {worst:.3f}")
    assert worst <= 1.0, (sr, worst)


def test_stereo_through_the_filter(tmp_path):
    p = write_wav(tmp_path / "st.wav", encode(clip_samples(3000, 2, seed=48), "s16"), "s16", 2, 48000)
    worst = error_ratio(_ref_of(p), p)
    print(f"48000 Hz stereo: largest error / bound = {worst:.3f}")
    assert worst <= 1.0, worst


def _frames_for(sr, n_out):
    """Input lengths whose output count is n_out (none where the rate cannot give it: at 8000 Hz the count is 3 n)."""
    return [n for n in range(1, 4 * n_out + 8) if api.intake_count(sr, n) == n_out]


def _edge_lengths(sr):
    ns = {1, 63}                                             # one frame; shorter than half the filter
    for want in (1, 255, 256, 257, 513):
        hits = _frames_for(sr, want)
        if not hits:                                         # not reachable at this rate: the next count above it that is
            assert sr == 8000 and want % 3 != 0
            hits = _frames_for(sr, want + 3 - want % 3)
        ns.add(hits[0])
    return sorted(ns)


@pytest.mark.parametrize("sr", [44100, 8000])
def test_tiles_and_edges(tmp_path, sr):
    """Output counts either side of one and two tiles of 256, a clip of one frame and one shorter than half the filter: the bound of
    test_against_host_resampler, and the same bits as the middle one of three clips of one launch."""
    lengths = _edge_lengths(sr)
    counts = [api.intake_count(sr, n) for n in lengths]
    if sr == 44100:
        assert {1, 255, 256, 257, 513} <= set(counts)
    else:
        assert {3, 255, 258, 513} <= set(counts)             # 8000 Hz: counts are multiples of 3
    other = encode(clip_samples(400, 2, seed=1), "s16")
    for n in lengths:
        raw = encode(clip_samples(n, 1, seed=n, sigma=0.3), "s16")
        p = write_wav(tmp_path / f"e{n}.wav", raw, "s16", 1, sr)
        got = _ref_of(p)
        assert got.size == api.intake_count(sr, n)
        worst = error_ratio(got, p)
        assert worst <= 1.0, (sr, n, worst)
        trio = api.RefAudio.many([(other, 16000, "s16", 2), (raw, sr, "s16"), (other, 48000, "s16", 2)])
        np.testing.assert_array_equal(_bits(trio[1].samples()), _bits(got), err_msg=f"{sr} Hz, {n} frames")
        for r in trio:
            r.close()


# ---------------------------------------------------------------- clips of one launch
def test_batch_is_independent():
    clips = [(encode(clip_samples(1500, 2, seed=1), "s16"), 44100, "s16", 2),
             (encode(clip_samples(700, 1, seed=2), "ulaw"), 8000, "ulaw", 1),
             (encode(clip_samples(900, 3, seed=3), "s24"), 24000, "s24", 3),
             (encode(clip_samples(2100, 8, seed=4), "f32"), 96000, "f32", 8),
             (encode(clip_samples(333, 1, seed=5), "u8"), 11025, "u8", 1)]
    many = api.RefAudio.many(clips)
    assert len(many) == 5
    for c, m in zip(clips, many):
        one = api.RefAudio.from_samples(*c)
        frames = len(c[0]) // (api.SRC_BYTES[api.SRC_NAMES.index(c[2])] * c[3])
        assert (m.source_rate, m.source_format, m.source_channels) == (c[1], c[2], c[3])
        assert len(m) == len(one) == api.intake_count(c[1], frames)
        np.testing.assert_array_equal(_bits(m.samples()), _bits(one.samples()), err_msg=c[2])
        one.close(); m.close()


def test_batch_is_all_or_nothing():
    keep = []
    good = api._clip_of(encode(clip_samples(200, 1, seed=1), "s16"), 16000, "s16", 1, keep)
    bad = api._clip_of(encode(clip_samples(200, 1, seed=1), "s16"), 44101, "s16", 1, keep)
    arr = (_lib.CClip * 5)(good, good, bad, good, good)
    hs = (ctypes.c_void_p * 5)()
    assert _lib.lib.q3_ref_audio_create_many(0, 5, arr, hs) == 7 and b"q3_resample" in _lib.lib.q3_last_error()
    assert not any(hs)
    with pytest.raises(_lib.Q3Error):
        api.RefAudio.many([(b"\0\0" * 50, 16000, "s16"), (b"\0\0" * 50, 16000, "s16"), (b"\0\0" * 50, 16000, "s16", 9)])
    rs = api.RefAudio.many([(b"\0\0" * 50, 16000, "s16")] * 2)      # ... and the next call is served
    assert [len(r) for r in rs] == [75, 75] and not rs[0].samples().any()
    for r in rs:
        r.close()
