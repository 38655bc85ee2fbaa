"""The keyed watermark on the host: the carrier, q3_mark_embed against a numpy float32 restatement of the step bit
for bit, q3_mark_detect against a numpy float64 restatement, the separation of marked and null scores around Q3_MARK_SCORE_DETECT,
the offset of a cut clip, and the refusals. No GPU. The restatements and the test signal are in mark_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
import mark_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3_INVALID_ARG = 1
T = api.MARK_SCORE_DETECT
KEYS = (0xC0FFEE, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF)
# (seed, seconds) of the separation's clips. At the default strength the 3 s clips of the measurement (profiles/mark_ab.txt) are all
# detected but do not all keep 1.5 x the threshold; 6 s and 10 s clips do, so those are the lengths here
CLIPS = [(21, 6.0), (22, 6.0), (23, 6.0), (24, 6.0), (25, 6.0), (26, 6.0), (31, 10.0), (32, 10.0), (33, 10.0)]


@pytest.fixture(scope="module")
def clips():
    out = {c: M.speechlike(*c) for c in CLIPS}
    for x in out.values():
        x.setflags(write=False)
    return out


def test_symbols_are_exported_bound_documented_and_in_the_shim():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    shim = open(os.path.join(ROOT, "shim", "src", "lib.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    for n in ("q3_pcm_stage_set_mark", "q3_mark_carrier", "q3_mark_embed", "q3_mark_detect", "q3_mark_score_detect", "q3_ref_audio_mark_score",
              "q3_session_set_mark", "q3_batcher_ticket_mark"):
        assert hasattr(_lib.lib, n) and n in _lib.SYMBOLS, n
        assert n in doc, n
        assert f"fn {n}(" in shim, n
        assert f" {n}(" in hdr, n
    m = re.search(r"#define Q3_MARK_SCORE_DETECT\s+([0-9.]+)", hdr)
    assert m and float(m.group(1)) == T == _lib.lib.q3_mark_score_detect()
    assert "#define Q3_MARK_STRENGTH_DEFAULT (-2600)" in hdr and api.mark_mb(api.MARK_DB_DEFAULT) == -2600


def test_carrier():
    cs = [M.carrier(k) for k in KEYS]
    for k, c in zip(KEYS, cs):
        assert (M.carrier(k).view(np.uint32) == c.view(np.uint32)).all()           # deterministic per key
        c64 = c.astype(np.float64)
        assert abs(np.sqrt(np.mean(c64 * c64)) - 1.0) <= 1e-6
        S = np.abs(np.fft.rfft(c64)) ** 2
        f = np.arange(S.size) * 24000.0 / M.P
        band = (f >= 500.0) & (f <= 3000.0)
        assert S[~band].sum() < 1e-9 * S.sum()
        assert S[band].min() > 0.5 * S[band].max()                                 # unit magnitude in every bin of the band
    for i in range(len(cs)):
        for j in range(i):
            a, b = cs[i].astype(np.float64), cs[j].astype(np.float64)
            assert abs(np.dot(a, b)) / M.P < 0.1                                   # other keys, other phases
    c = np.zeros(M.P, np.float32)
    assert _lib.lib.q3_mark_carrier(0, c.ctypes.data_as(ctypes.c_void_p)) == Q3_INVALID_ARG
    assert _lib.lib.q3_mark_carrier(5, None) == Q3_INVALID_ARG
    assert (api.mark_carrier("c0ffee").view(np.uint32) == cs[0].view(np.uint32)).all()


def test_ramp_is_one_rounding_either_way():
    """(float)(j / 240.0), the header's weight, is also the correctly rounded f32 quotient the kernel takes"""
    j = np.arange(M.H)
    assert ((j / 240.0).astype(np.float32) == (j.astype(np.float32) / np.float32(240.0))).all()


@pytest.mark.parametrize("strength", [-2600, -4000, -1000])
def test_embed_is_the_restatement_bitwise(strength):
    """2 s with a stretch of digital silence, a NaN and an inf, a length that is no multiple of the hop"""
    x = M.speechlike(5, 2.0)[:47917].copy()
    x[9000:15000] = 0.0
    x[20001] = np.nan; x[30007] = np.inf; x[30500] = -np.inf
    want = M.embed_ref(x, KEYS[0], strength)
    got = M.lib_embed(x, KEYS[0], strength)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert np.isnan(got[20001]) and np.isinf(got[30007])                           # a non-finite sample leaves as it came
    d = got[:9000].astype(np.float64) - x[:9000].astype(np.float64)
    assert d.std() > 0                                                             # (something was added)
    np.testing.assert_array_equal(got[9000 + 3 * M.H:15000], 0.0)                  # nothing under digital silence, two hops behind its start
    assert (api.mark_embed(x, KEYS[0], strength / 100.0).view(np.uint32) == want.view(np.uint32)).all()


def test_embed_level_follows_the_signal():
    x = M.speechlike(6, 3.0)
    for db in (-20.0, -30.0):
        y = api.mark_embed(x, 77, db)
        d = (y.astype(np.float64) - x.astype(np.float64))[2 * M.H:]
        ratio = 10.0 * np.log10(np.mean(d * d) / np.mean(x[2 * M.H:].astype(np.float64) ** 2))
        assert abs(ratio - db) < 2.0, (db, ratio)


def test_detect_is_the_restatement(clips):
    for (seed, sec), x in clips.items():
        if sec != 6.0:
            continue
        y = M.lib_embed(x, KEYS[0])
        for z, k in ((y, KEYS[0]), (x, KEYS[0]), (y[777:100001], KEYS[0]), (y, KEYS[1])):
            s, off = M.lib_detect(z, k)
            rs, roff, _ = M.detect_ref(z, k)
            assert off == roff
            assert abs(s - rs) <= 1e-9 * abs(rs), (s, rs)
    z = clips[(21, 6.0)].copy()
    z[100] = np.nan; z[5000] = np.inf; z[30000:40000] = 0.0
    s, off = M.lib_detect(z, 9)
    rs, roff, _ = M.detect_ref(z, 9)
    assert off == roff and abs(s - rs) <= 1e-9 * abs(rs)
    r = api.mark_detect(api.AudioBuffer(y, 24000), KEYS[0])
    assert r.detected and r.offset == 0 and r.score == M.lib_detect(y, KEYS[0])[0]


def test_separation(clips):
    """every marked score >= 1.5 x the threshold, every null score (unmarked, and marked with another key) <= threshold / 1.5"""
    for i, ((seed, sec), x) in enumerate(clips.items()):
        key, other = KEYS[i % len(KEYS)], KEYS[(i + 1) % len(KEYS)]
        y = M.lib_embed(x, key)
        marked = M.lib_detect(y, key)[0]
        nulls = (M.lib_detect(x, key)[0], M.lib_detect(y, other)[0], M.lib_detect(M.lib_embed(x, other), key)[0])
        print(f"seed {seed} {sec:g} s: marked {marked:.2f}, nulls {nulls[0]:.2f} {nulls[1]:.2f} {nulls[2]:.2f}, threshold {T}")
        assert marked >= 1.5 * T, (seed, sec, marked)
        assert max(nulls) <= T / 1.5, (seed, sec, nulls)


@pytest.mark.parametrize("cut", [1, 239, 4095, 4096, 12345, 50001])
def test_offset_of_a_cut_clip(clips, cut):
    y = M.lib_embed(clips[(22, 6.0)], KEYS[3])
    s, off = M.lib_detect(y[cut:], KEYS[3])
    assert off == cut % M.P and s >= 1.5 * T


def test_refusals():
    L = _lib.lib
    x = np.zeros(3 * M.P, np.float32); y = np.zeros_like(x)
    px, py = x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p)
    sc = ctypes.c_double(); off = ctypes.c_int()
    for mb in (-4001, -999, 0, 2000):
        assert L.q3_mark_embed(px, x.size, 5, mb, py) == Q3_INVALID_ARG
        assert L.q3_last_error() == f"q3_mark_embed: strength {mb} mB out of range (-4000..-1000)".encode()
    assert L.q3_mark_embed(px, x.size, 0, -2000, py) == Q3_INVALID_ARG and b"key 0 is off" in L.q3_last_error()
    assert L.q3_mark_embed(None, x.size, 5, -2000, py) == Q3_INVALID_ARG
    assert L.q3_mark_embed(px, 0, 5, -2000, py) == 0                               # an empty clip is a clip
    assert L.q3_mark_detect(px, 2 * M.P - 1, 5, ctypes.byref(sc), ctypes.byref(off)) == Q3_INVALID_ARG
    assert b"at least 8192" in L.q3_last_error()
    assert L.q3_mark_detect(px, x.size, 0, ctypes.byref(sc), ctypes.byref(off)) == Q3_INVALID_ARG
    assert L.q3_mark_detect(None, x.size, 5, ctypes.byref(sc), ctypes.byref(off)) == Q3_INVALID_ARG
    assert L.q3_mark_detect(px, x.size, 5, None, None) == Q3_INVALID_ARG
    assert L.q3_mark_detect(px, 2 * M.P, 5, ctypes.byref(sc), ctypes.byref(off)) == 0 and sc.value == 0.0      # digital silence scores nothing
    # the setters refuse before the device is touched: a null handle is the refusal here (no device), the range is the stage's
    assert L.q3_pcm_stage_set_mark(None, 0, 5, -2000) == Q3_INVALID_ARG
    assert L.q3_session_set_mark(None, 0, 5, -2000) == Q3_INVALID_ARG
    assert L.q3_batcher_ticket_mark(None, 0, 5, -2000) == Q3_INVALID_ARG
    assert L.q3_ref_audio_mark_score(None, 5, ctypes.byref(sc), ctypes.byref(off)) == Q3_INVALID_ARG
    with pytest.raises(ValueError):
        api.mark_key("xyz")
    with pytest.raises(ValueError):
        api.mark_key(1 << 64)
    with pytest.raises(ValueError):
        api.mark_embed(api.AudioBuffer(x, 16000), 5)


def test_cli_flags_refuse_before_anything_is_loaded():
    from qwen3_tts_rs_amd import cli
    ap = cli.build_parser()
    for argv, word in ((["--watermark-key", "c0ffee"], "--streaming"), (["--streaming", "--watermark-db", "-30"], "--watermark-key"),
                       (["--streaming", "--watermark-key", "zz"], "hexadecimal"), (["--streaming", "--watermark-key", "0"], "off"),
                       (["--streaming", "--watermark-key", "1", "--watermark-db", "-5"], "out of range")):
        with pytest.raises(ValueError) as e:
            cli.mark_from_args(ap.parse_args(argv))
        assert word in str(e.value), (argv, str(e.value))
    assert cli.mark_from_args(ap.parse_args([])) is None
    assert cli.mark_from_args(ap.parse_args(["--streaming", "--watermark-key", "0xC0FFEE"])) == (0xC0FFEE, -26.0)


def test_cli_detects_on_the_host(tmp_path, capsys):
    """--detect-watermark with the host intake: a marked 16 kHz WAV reports a detection, the same file under another key none"""
    from qwen3_tts_rs_amd import cli
    y = M.lib_embed(M.speechlike(41, 6.0), 0xC0FFEE)
    p = str(tmp_path / "marked.wav")
    api.save_wav(p, api.resample(api.AudioBuffer(y, 24000), 16000).samples, 16000)
    assert cli.main(["--detect-watermark", "c0ffee", p]) == 0
    out = capsys.readouterr().out
    assert ": DETECTED" in out and "offset 0," in out
    assert cli.main(["--detect-watermark", "c0ffef", p]) == 0
    assert "not detected" in capsys.readouterr().out
    assert cli.main(["--detect-watermark", "c0ffee", str(tmp_path / "missing.wav")]) == 2
