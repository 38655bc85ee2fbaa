"""Shared by the watermark tests and tools/dev/mark_ab.py: the seeded speech-like test signal, numpy restatements of the embed
step (float32, include/q3tts.h's operations in their order) and of the detector (float64), and the host round trip through the
stage's own formats."""
import ctypes

import numpy as np

P, H = 4096, 240
F32 = np.float32


def speechlike(seed, seconds, rate=24000):
    """Harmonic stacks under a syllabic envelope, with pauses and a noise floor: syllables of 110..300 ms on a pitch contour of
    85..230 Hz, harmonics up to 4.2 kHz under a spectral tilt and two moving formant bumps, phrases of 3..9 syllables parted by
    pauses of 150..600 ms, a noise floor at -62 dBFS, peak about 0.35. float32, deterministic per seed."""
    rng = np.random.default_rng(seed)
    n = int(round(seconds * rate))
    x = np.zeros(n, np.float64)
    t0 = int(rng.integers(0, rate // 5))
    while t0 < n:
        f0 = rng.uniform(85.0, 230.0)
        for _ in range(int(rng.integers(3, 10))):
            ln = int(rng.uniform(0.11, 0.30) * rate)
            if t0 >= n:
                break
            m = min(ln, n - t0)
            tt = np.arange(m) / rate
            f0 = float(np.clip(f0 * rng.uniform(0.92, 1.09), 85.0, 230.0))
            glide = rng.uniform(-0.08, 0.08)
            ph = 2.0 * np.pi * f0 * (tt + 0.5 * glide * tt * tt / max(ln / rate, 1e-3))
            f1, f2 = rng.uniform(300.0, 900.0), rng.uniform(1000.0, 2600.0)
            amp = rng.uniform(0.25, 1.0)
            env = np.sin(np.pi * (np.arange(m) + 0.5) / ln) ** 2
            syl = np.zeros(m)
            for k in range(1, int(4200.0 / f0) + 1):
                fk = k * f0
                a = (1.0 / k) * (1.0 + 3.0 * np.exp(-((fk - f1) / 160.0) ** 2) + 2.0 * np.exp(-((fk - f2) / 260.0) ** 2))
                syl += a * np.sin(k * ph + rng.uniform(0.0, 2.0 * np.pi))
            if rng.random() < 0.25:                                   # an unvoiced onset
                fr = min(m, int(0.04 * rate))
                syl[:fr] += 2.0 * rng.standard_normal(fr)
            x[t0:t0 + m] += amp * env * syl
            t0 += ln + int(rng.uniform(0.0, 0.04) * rate)
        t0 += int(rng.uniform(0.15, 0.6) * rate)
    pk = np.max(np.abs(x))
    if pk > 0:
        x *= 0.35 / pk
    x += 10.0 ** (-62.0 / 20.0) * rng.standard_normal(n)
    return x.astype(F32)


def carrier(key):
    from qwen3_tts_rs_amd import _lib
    c = np.zeros(P, F32)
    _lib.check(_lib.lib.q3_mark_carrier(ctypes.c_uint64(key), c.ctypes.data_as(ctypes.c_void_p)))
    return c


def hop_energy_f32(v):
    """e_h of one whole hop: 64 interleaved float32 partials, sample j to partial j mod 64 in ascending j, folded d = 32 .. 1"""
    v = np.where(np.isfinite(v), v, F32(0)).astype(F32)
    sq = (v * v).astype(F32)
    p = np.zeros(64, F32)
    for j0 in range(0, H, 64):
        seg = sq[j0:j0 + 64]
        p[:seg.size] = (p[:seg.size] + seg).astype(F32)
    d = 32
    while d >= 1:
        p[:d] = (p[:d] + p[d:2 * d]).astype(F32)
        d >>= 1
    return p[0]


def embed_ref(x, key, strength_mb, c=None):
    """the embed step in numpy float32: every operation rounded once, in the header's order"""
    x = np.asarray(x, F32)
    c = carrier(key) if c is None else c
    s = F32(10.0 ** (strength_mb / 2000.0))
    ramp = (np.arange(H) / 240.0).astype(F32)
    inv = F32(1.0 / 240.0)
    y = np.empty_like(x)
    r1 = r2 = F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for h0 in range(0, x.size, H):
            hop = x[h0:h0 + H]
            m = hop.size
            g = (r2 + ((r1 - r2).astype(F32) * ramp[:m]).astype(F32)).astype(F32)
            idx = (h0 + np.arange(m)) % P
            y[h0:h0 + m] = (hop + ((s * g).astype(F32) * c[idx]).astype(F32)).astype(F32)
            if m == H:
                r2, r1 = r1, np.sqrt((hop_energy_f32(hop) * inv).astype(F32)).astype(F32)
    return y


def detect_ref(z, key, c=None):
    """the detector in numpy float64 -> (score, offset, rho)"""
    z = np.asarray(z, F32)
    c = (carrier(key) if c is None else c).astype(np.float64)
    v = np.where(np.isfinite(z), z, 0).astype(np.float64)
    nh = (v.size + H - 1) // H
    pad = np.zeros(nh * H)
    pad[:v.size] = v
    r = np.maximum(np.sqrt((pad.reshape(nh, H) ** 2).sum(axis=1) / 240.0), 1e-4)
    zn = (pad.reshape(nh, H) / r[:, None]).reshape(-1)[:v.size]
    nk = (v.size + P - 1) // P
    fold = np.zeros(nk * P)
    fold[:v.size] = zn
    Fm = fold.reshape(nk, P).sum(axis=0)
    # rho[d] = sum_m F[m] c[(m + d) mod P]: a cyclic cross-correlation
    rho = np.fft.irfft(np.conj(np.fft.rfft(Fm)) * np.fft.rfft(c), P)
    d = int(np.argmax(rho))
    return float((rho[d] - rho.mean()) / rho.std()), d, rho


def lib_embed(x, key, strength_mb=-2600):
    from qwen3_tts_rs_amd import _lib
    x = np.ascontiguousarray(x, F32)
    y = np.zeros_like(x)
    _lib.check(_lib.lib.q3_mark_embed(x.ctypes.data_as(ctypes.c_void_p), x.size, ctypes.c_uint64(key), int(strength_mb), y.ctypes.data_as(ctypes.c_void_p)))
    return y


def lib_detect(z, key):
    from qwen3_tts_rs_amd import _lib
    z = np.ascontiguousarray(z, F32)
    sc = ctypes.c_double(); off = ctypes.c_int()
    _lib.check(_lib.lib.q3_mark_detect(z.ctypes.data_as(ctypes.c_void_p), z.size, ctypes.c_uint64(key), ctypes.byref(sc), ctypes.byref(off)))
    return sc.value, off.value


def host_round_trip(y, rate, fmt):
    """A 24 kHz clip through the stage's own formats on the CPU: q3_resample to `rate`, PCM16 (fmt "s16") or G.711 mu-law of it
    (fmt "ulaw") with the host helpers, back to float32 (the intake's scale, 2^-15) and q3_resample to 24 kHz."""
    from qwen3_tts_rs_amd import api, _lib
    a = api.resample(api.AudioBuffer(np.ascontiguousarray(y, F32), 24000), rate).samples
    pcm = np.zeros(a.size, np.int16)
    _lib.check(_lib.lib.q3_pcm16_from_f32(a.ctypes.data_as(ctypes.c_void_p), a.size, pcm.ctypes.data_as(ctypes.c_void_p)))
    if fmt == "ulaw":
        pcm = api.g711_expand(api.g711(pcm, "ulaw"), "ulaw")
    back = (pcm.astype(F32) * F32(2.0 ** -15)).astype(F32)
    return api.resample(api.AudioBuffer(back, rate), 24000).samples
