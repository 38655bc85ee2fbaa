"""G.711 out of the output stage: Q3_PCM_ULAW / Q3_PCM_ALAW are the ITU-T G.711 companding of the int16 value that
Q3_PCM_S16 writes for the same sample, one byte per sample. The yardstick is tests/golden/g711_tables.npz — CPython's `audioop`
over every int16 value (tests/make_golden_g711.py) —, held against `audioop` itself where it imports and against a numpy
restatement of the two formulas. Host parts run anywhere; the `gpu` tests feed one stage synthetic PCM, no model."""
import ctypes
import os
import struct

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api

NEW = ["q3_g711_from_pcm16", "q3_wav_write_g711"]
Q3_INVALID_ARG = 1
LAWS = ["ulaw", "alaw"]
ZERO_BYTE = {"ulaw": 0xFF, "alaw": 0xD5}


@pytest.fixture(scope="module")
def table():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz"))
    t = {"ulaw": z["ulaw"].copy(), "alaw": z["alaw"].copy()}
    for a in t.values():
        assert a.dtype == np.uint8 and a.shape == (65536,)
        a.setflags(write=False)
    return t


# ---------------------------------------------------------------- the two formulas, restated on 64-bit integers
def _seg(p, bounds):
    """first index whose bound is >= p, 8 if none"""
    return np.searchsorted(np.asarray(bounds, dtype=np.int64), p, side="left")


def np_ulaw(v):
    v = np.asarray(v, dtype=np.int64)
    p = v >> 2
    mask = np.where(p < 0, 0x7F, 0xFF)
    p = np.where(p < 0, -p, p)
    p = np.minimum(p, 8159) + 33
    seg = _seg(p, [0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])
    body = np.where(seg == 8, 0x7F, (seg << 4) | ((p >> (np.minimum(seg, 7) + 1)) & 0xF))
    return (body ^ mask).astype(np.uint8)


def np_alaw(v):
    v = np.asarray(v, dtype=np.int64)
    p = v >> 3
    mask = np.where(p >= 0, 0xD5, 0x55)
    p = np.where(p >= 0, p, -p - 1)
    seg = _seg(p, [0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF])
    s7 = np.minimum(seg, 7)
    body = np.where(seg == 8, 0x7F, (seg << 4) | np.where(seg < 2, (p >> 1) & 0xF, (p >> s7) & 0xF))
    return (body ^ mask).astype(np.uint8)


ALL16 = np.arange(-32768, 32768, dtype=np.int64)


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(api.g711) and callable(api.save_wav_g711)
    assert (api.PCM_ULAW, api.PCM_ALAW) == (2, 3)


def test_null_and_bad_arguments_give_a_status_and_a_message():
    L = _lib.lib
    one = np.zeros(1, np.int16); out = np.zeros(1, np.uint8)
    pi, po = one.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    for f in (lambda: L.q3_g711_from_pcm16(None, 1, 2, po), lambda: L.q3_g711_from_pcm16(pi, 1, 2, None),
              lambda: L.q3_g711_from_pcm16(pi, 1, 1, po), lambda: L.q3_g711_from_pcm16(pi, 1, 4, po), lambda: L.q3_g711_from_pcm16(pi, -1, 2, po),
              lambda: L.q3_wav_write_g711(None, po, 1, 8000, 2), lambda: L.q3_wav_write_g711(b"x.wav", None, 1, 8000, 2),
              lambda: L.q3_wav_write_g711(b"x.wav", po, 1, 8000, 0), lambda: L.q3_wav_write_g711(b"x.wav", po, 1, 8000, 1)):
        assert f() == Q3_INVALID_ARG and len(L.q3_last_error()) > 0
    assert L.q3_wav_write_g711(b"no-such-dir/x.wav", po, 1, 8000, 2) != 0 and len(L.q3_last_error()) > 0
    with pytest.raises(ValueError):
        api.g711(one, "s16")


@pytest.mark.parametrize("law", LAWS)
def test_host_helper_equals_the_fixture_over_all_inputs(table, law):
    np.testing.assert_array_equal(api.g711(ALL16.astype(np.int16), law), table[law])


def test_fixture_equals_audioop(table):
    audioop = pytest.importorskip("audioop")
    raw = ALL16.astype("<i2").tobytes()
    np.testing.assert_array_equal(np.frombuffer(audioop.lin2ulaw(raw, 2), np.uint8), table["ulaw"])
    np.testing.assert_array_equal(np.frombuffer(audioop.lin2alaw(raw, 2), np.uint8), table["alaw"])


def test_numpy_restatement_equals_the_fixture(table):
    np.testing.assert_array_equal(np_ulaw(ALL16), table["ulaw"])
    np.testing.assert_array_equal(np_alaw(ALL16), table["alaw"])
    assert table["ulaw"][32768] == 0xFF and table["alaw"][32768] == 0xD5


def parse_wav(path):
    """RIFF chunks by struct.unpack: {"fmt": (tag, channels, rate, byte rate, align, bits, cbSize or None), "fact": n, "data": bytes}"""
    b = open(path, "rb").read()
    riff, size, wave_ = struct.unpack("<4sI4s", b[:12])
    assert riff == b"RIFF" and wave_ == b"WAVE" and size == len(b) - 8
    out = {}; off = 12
    while off + 8 <= len(b):
        cid, n = struct.unpack("<4sI", b[off:off + 8])
        body = b[off + 8:off + 8 + n]
        assert len(body) == n
        if cid == b"fmt ":
            out["fmt_len"] = n
            out["fmt"] = struct.unpack("<HHIIHH", body[:16]) + ((struct.unpack("<H", body[16:18])[0],) if n >= 18 else (None,))
        elif cid == b"fact":
            out["fact"] = struct.unpack("<I", body[:4])[0]
        elif cid == b"data":
            out["data"] = body
        off += 8 + n + (n & 1)
    assert off == len(b)
    return out


@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [0, 1, 801, 8000])
def test_wav_write_g711_header(tmp_path, law, tag, n):
    rng = np.random.default_rng(n)
    data = rng.integers(0, 256, size=n).astype(np.uint8)
    p = tmp_path / f"{law}.wav"
    api.save_wav_g711(str(p), data, 8000, law)
    w = parse_wav(str(p))
    assert w["fmt_len"] == 18
    assert w["fmt"] == (tag, 1, 8000, 8000, 1, 8, 0)
    assert w["fact"] == n and len(w["data"]) == n
    assert w["data"] == data.tobytes()
    # q3_wav_read stays as it is: it takes PCM and float
    cnt = ctypes.c_int64(); rate = ctypes.c_uint32()
    assert _lib.lib.q3_wav_read(str(p).encode(), None, 0, ctypes.byref(cnt), ctypes.byref(rate)) != 0


def test_formats_out_of_range_are_refused():
    L = _lib.lib
    for fmt in (-1, 4, 7):
        assert L.q3_pcm_stage_set(None, 0, 8000, fmt) == Q3_INVALID_ARG
        assert L.q3_session_set_output(None, 8000, fmt) == Q3_INVALID_ARG
        assert L.q3_batcher_ticket_output(None, 1, 8000, fmt) == Q3_INVALID_ARG
    with pytest.raises(ValueError):
        api.pcm_format(True, "ulaw")                       # pcm16= and fmt= together
    with pytest.raises(ValueError):
        api.pcm_format(False, "u8")
    assert [api.pcm_format(fmt=f) for f in ("f32", "s16", "ulaw", "alaw")] == [0, 1, 2, 3]
    assert api.pcm_format(True) == 1 and api.pcm_format() == 0


# ---------------------------------------------------------------- GPU, synthetic PCM, no model
def ramp():
    """x = (v +- 0.25) / 32767, + for v >= 0: the S16 rule returns exactly v, every reachable int16 value once"""
    v = np.arange(-32767, 32768, dtype=np.int64)
    x = (v.astype(np.float64) + np.where(v >= 0, 0.25, -0.25)) / 32767.0
    return v, x.astype(np.float32)


def speech_like():
    rng = np.random.default_rng(711)
    n = 24000
    t = np.arange(n) / 24000.0
    ph = 2.0 * np.pi * np.cumsum(np.linspace(110.0, 170.0, n)) / 24000.0
    x = sum(np.sin(k * ph) / k for k in range(1, 7)) * 0.45 * (0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t)) + 0.01 * rng.standard_normal(n)
    x[9000:10000] = 0.0
    return x.astype(np.float32)


def run_row(ps, row, x, piece):
    out = []; at = 0
    while True:
        n = min(piece, x.size - at); last = at + n >= x.size
        out.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
        if last:
            return np.concatenate(out)


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 3, 65535)
    yield ps
    ps.close()


@pytest.mark.gpu
def test_format_2_is_accepted_and_4_refused(stage):
    stage.set(0, 24000, fmt="ulaw"); stage.set(0, 24000, fmt="alaw")
    assert stage.dtype(0) == np.uint8
    assert _lib.lib.q3_pcm_stage_set(stage._h, 0, 24000, 4) == Q3_INVALID_ARG
    stage.set(0, 24000)


@pytest.mark.gpu
def test_ramp_at_24k_covers_every_value_and_equals_the_table(stage, table):
    v, x = ramp()
    stage.set(0, 24000, fmt="s16")
    s16 = run_row(stage, 0, x, x.size)
    assert s16.dtype == np.int16
    np.testing.assert_array_equal(s16, v)                  # all 65 535 reachable values, in order
    np.testing.assert_array_equal(s16, api.pcm16(x))
    for law in LAWS:
        stage.set(0, 24000, fmt=law)
        g = run_row(stage, 0, x, 20000)                    # (four pushes: more than one tile, a last one that is not whole)
        assert g.dtype == np.uint8 and g.size == x.size
        np.testing.assert_array_equal(g, table[law][s16.astype(np.int64) + 32768], err_msg=law)


@pytest.mark.gpu
def test_nan_gives_the_byte_of_zero(stage):
    x = np.array([0.5, np.nan, -0.5, np.inf, -np.inf, 0.0, -0.0], np.float32)
    for law in LAWS:
        stage.set(0, 24000, fmt=law)
        g = run_row(stage, 0, x, x.size)
        assert g[1] == ZERO_BYTE[law] and g[5] == ZERO_BYTE[law] and g[6] == ZERO_BYTE[law]
        np.testing.assert_array_equal(g, api.g711(api.pcm16(x), law))


@pytest.mark.gpu
def test_8k_equals_the_table_of_the_s16_run(stage, table):
    x = speech_like()
    stage.set(0, 8000, fmt="s16")
    s16 = run_row(stage, 0, x, 1920)
    assert s16.size == 8000 and np.unique(s16).size > 2000
    for law in LAWS:
        stage.set(0, 8000, fmt=law)
        g = run_row(stage, 0, x, 1920)
        np.testing.assert_array_equal(g, table[law][s16.astype(np.int64) + 32768], err_msg=law)
        np.testing.assert_array_equal(api.resample_gpu(x, 8000, fmt=law).samples, g)


@pytest.mark.gpu
def test_three_rows_three_formats_one_stage(stage):
    """Rows at s16 / ulaw / alaw with different push sizes (and rates) in one push sequence against their one-row runs."""
    x = speech_like()
    cfg = {0: (8000, "s16", 1920, x), 1: (8000, "ulaw", 1000, x[:9001]), 2: (16000, "alaw", 2501, x[:17000])}
    solo = api.PcmStage(0, 1, 24000)
    want = {}
    for r, (sr, f, piece, sig) in cfg.items():
        solo.set(0, sr, fmt=f)
        want[r] = run_row(solo, 0, sig, piece)
    solo.close()
    for r, (sr, f, piece, sig) in cfg.items():
        stage.set(r, sr, fmt=f)
    at = {r: 0 for r in cfg}; got = {r: [] for r in cfg}
    while any(at[r] < cfg[r][3].size for r in cfg):
        push = {}; last = []
        for r, (sr, f, piece, sig) in cfg.items():
            if at[r] >= sig.size:
                continue
            n = min(piece, sig.size - at[r])
            push[r] = sig[at[r]:at[r] + n]; at[r] += n
            if at[r] >= sig.size:
                last.append(r)
        out = stage.push(push, last=tuple(last))
        for r in push:
            got[r].append(out[r])
    for r in cfg:
        g = np.concatenate(got[r])
        assert g.dtype == want[r].dtype
        np.testing.assert_array_equal(g, want[r], err_msg=f"row {r}")
