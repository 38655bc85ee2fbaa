"""The formant step's definition (include/q3tts.h at q3_pcm_stage_set_formant) restated in float64, the probe signal
its tests share, and the band centroid they measure. The restatement is the reference of tests/test_formant_host.py and
tests/test_gpu_formant.py; it takes the warp omega as the stage's descriptor carries it (float32, from q3_pcm_stage_formant_plan)."""
import numpy as np

N, H, LIFT = 1024, 256, 40
CLAMP = float(np.log(10.0 ** (18.0 / 20.0)))
RATE = 24000


def window():
    return np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N))


def formant_ref(x, omega):
    """The whole row at once: frames m = 0 .. ceil(n / H) + 2 over samples [H m - 768, H m + 256), zeros outside [0, n)."""
    x = np.asarray(x, np.float64)
    n = x.size
    if n == 0:
        return x
    w, om = window(), float(np.float32(omega))
    frames = -(-n // H) + 3
    xp = np.concatenate([np.zeros(N - H), x, np.zeros(frames * H + H - n)])
    X = np.fft.rfft(xp[np.arange(frames)[:, None] * H + np.arange(N)[None, :]] * w, axis=1)
    c = np.fft.irfft(0.5 * np.log(np.maximum(np.abs(X) ** 2, 1e-12)), n=N, axis=1)
    c[:, LIFT + 1:N - LIFT] = 0.0
    E = np.fft.rfft(c, axis=1).real
    u = np.arange(N // 2 + 1) * om
    i = np.minimum(np.floor(u).astype(np.int64), N // 2 - 1)
    Ew = np.where(u >= N // 2, E[:, N // 2:], E[:, i] + (u - i) * (E[:, i + 1] - E[:, i]))
    y = np.fft.irfft(np.exp(np.clip(Ew - E, -CLAMP, CLAMP)) * X, n=N, axis=1) * w
    out = np.zeros(xp.size)
    for m in range(frames):                                    # ascending m
        out[m * H:m * H + N] += y[m]
    return 0.5 * out[N - H:N - H + n]


def envelope(f):
    """The probe's spectral envelope: three resonances near 700 / 1200 / 2600 Hz on a floor."""
    f = np.asarray(f, np.float64)
    return (1.0 * np.exp(-0.5 * ((f - 700.0) / 110.0) ** 2) + 0.7 * np.exp(-0.5 * ((f - 1200.0) / 130.0) ** 2) +
            0.4 * np.exp(-0.5 * ((f - 2600.0) / 200.0) ** 2) + 0.02)


def vowel(f0=120.0, warp=1.0, seconds=0.3, seed=7):
    """A synthetic vowel at 24 kHz: harmonics of f0 under envelope(f / warp), plus a little seeded noise so that no bin is empty.
    warp = p with f0 = 120 p is what varispeed by p (and a stretch back) makes of the vowel at f0 = 120."""
    n = int(round(seconds * RATE))
    t = np.arange(n) / RATE
    k = np.arange(1, int(0.45 * RATE / f0) + 1)
    x = (envelope(k * f0 / warp)[:, None] * np.sin(2.0 * np.pi * f0 * k[:, None] * t[None, :] + 0.7 * k[:, None] ** 2)).sum(axis=0)
    x = 0.25 * x / np.abs(x).max() + 1e-4 * np.random.default_rng(seed).standard_normal(n)
    return x.astype(np.float32)


def band_centroid(x, lo=300.0, hi=1100.0):
    """The spectral centroid in Hz of [lo, hi] of the long-term power spectrum (Hann frames of 2048, hop 512, averaged)."""
    x = np.asarray(x, np.float64)
    L = 2048
    idx = np.arange(0, x.size - L + 1, 512)[:, None] + np.arange(L)[None, :]
    P = (np.abs(np.fft.rfft(x[idx] * np.hanning(L), axis=1)) ** 2).mean(axis=0)
    f = np.arange(L // 2 + 1) * RATE / L
    band = (f >= lo) & (f <= hi)
    return float((f[band] * P[band]).sum() / P[band].sum())
