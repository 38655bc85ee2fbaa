"""Shared by the intake tests (test_intake_host.py, test_gpu_intake.py, test_intake_layers.py): WAV files written
by hand in every sample format the intake reads, the f64 restatement of its table, and the rounding bound of its dot product."""
import math
import struct

import numpy as np

from qwen3_tts_rs_amd import api

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000]
LM = {8000: (3, 1), 11025: (320, 147), 16000: (3, 2), 22050: (160, 147), 32000: (3, 4), 44100: (80, 147), 48000: (1, 2), 96000: (1, 4)}
FORMATS = {"u8": (1, 8), "s16": (1, 16), "s24": (1, 24), "s32": (1, 32), "f32": (3, 32), "ulaw": (7, 8), "alaw": (6, 8)}      # WAVE tag, bits


def encode(x, fmt):
    """x: float64 in [-1, 1], any shape -> the on-disk bytes of `fmt`, interleaved in x's own (C) order. Full scale included."""
    x = np.asarray(x, dtype=np.float64)
    if fmt == "f32":
        return x.astype("<f4").tobytes()
    if fmt == "u8":
        return (np.clip(np.rint(x * 128.0), -128, 127) + 128).astype(np.uint8).tobytes()
    if fmt == "s16":
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2").tobytes()
    if fmt == "s32":
        return np.clip(np.rint(x * 2147483648.0), -2147483648, 2147483647).astype("<i4").tobytes()
    if fmt == "s24":
        v = np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype(np.int64).reshape(-1) & 0xFFFFFF
        return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    s16 = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16).reshape(-1)
    return api.g711(s16, fmt).tobytes()


def clip_samples(frames, channels, seed, sigma=0.3):
    """Finite random samples with full-scale values among them, [frames, channels] f64."""
    rng = np.random.default_rng(seed)
    x = np.clip(sigma * rng.standard_normal((frames, channels)), -1.0, 1.0)
    flat = x.reshape(-1)
    flat[:: max(1, flat.size // 7)] = 1.0
    flat[1:: max(1, flat.size // 5)] = -1.0
    return x


def write_wav(path, raw, fmt, channels, rate, front=b"", extensible=False):
    """A RIFF/WAVE file around `raw`. front: bytes of whole chunks to put between `fmt ` and `data` (their own padding included)."""
    tag, bits = FORMATS[fmt]
    block = channels * bits // 8
    if extensible:      # WAVE_FORMAT_EXTENSIBLE: cbSize 22, valid bits, channel mask, sub-format GUID whose first two bytes are the tag
        body = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, 0) + \
            struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    elif tag in (6, 7):
        body = struct.pack("<HHIIHHH", tag, channels, rate, rate * block, block, bits, 0)
    else:
        body = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    chunks = b"fmt " + struct.pack("<I", len(body)) + body + front + b"data" + struct.pack("<I", len(raw)) + raw + (b"\0" if len(raw) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return str(path)


def chunk(name, payload):
    """One RIFF chunk, padded to an even length as the format asks."""
    return name + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def np_taps(sr):
    """The window-sinc of q3_resample (q3_io.cpp) at t - c = p / L for sr_in = sr, sr_out = 24000, in f64."""
    g = math.gcd(sr, 24000); L, M = 24000 // g, sr // g
    fc = 0.95 * min(L / M, 1.0)
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


def host_24k(path):
    """Today's path: q3_wav_read, then q3_resample to 24 kHz."""
    return api.resample_to_24k(api.load_wav(str(path))).samples


def error_ratio(got, path):
    """Largest |got - host| / (132 * 2^-24 * sum_j |h[p][j]| |x[c - 63 + j]|) over EVERY output sample of the clip in `path`, with h
    from q3_intake_taps and x the mono stream q3_wav_read gives: one rounding per tap, 128 products, 127 additions and the host's
    final cast (the bound of tests/test_pcm_stage.py, for the input direction). Lengths must agree."""
    mono = api.load_wav(str(path))
    ref = api.resample_to_24k(mono).samples
    assert got.shape == ref.shape, (got.shape, ref.shape)
    h, L, M = api.intake_taps(mono.sample_rate)
    i = np.arange(got.size, dtype=np.int64)
    c, p = (i * M) // L, (i * M) % L
    pad = int(c.max()) + 65 + 1
    xpad = np.zeros(63 + max(pad, mono.samples.size + 1))
    xpad[63:63 + mono.samples.size] = np.abs(mono.samples.astype(np.float64))
    idx = c[:, None] + np.arange(128)[None, :]            # input c - 63 + j sits at xpad[c + j]
    mag = (np.abs(h.astype(np.float64))[p] * xpad[idx]).sum(axis=1)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = 132.0 * 2.0 ** -24 * mag
    assert (err[bound == 0.0] == 0.0).all()
    return float((err / np.maximum(bound, 1e-300)).max())
