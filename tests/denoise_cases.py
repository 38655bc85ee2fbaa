"""The spectral noise suppressor's definition (include/q3tts.h, q3_ref_audio_denoise) restated in float64, and the probe signal of
its tests: three gated tones plus seeded Gaussian noise."""
import numpy as np

N, H, K, D, C_BIAS = 512, 128, 257, 94, 4.0
LENGTHS = [1, 127, 128, 129, 384, 385, 511, 513, 24000, 25111]


def plan(n):
    """(T, lo, hi, workspace bytes)"""
    T = -(-n // H) + 3
    return T, 3, T - 4, 16 * T * K


def probe(n, seed=0):
    """(noisy, clean) float32: tones of 220 / 440 / 1760 Hz, amplitude 0.3, gated by sin(2 pi 1.5 t) > 0.2, noise of sigma 0.02"""
    t = np.arange(n) / 24000.0
    gate = (np.sin(2 * np.pi * 1.5 * t) > 0.2).astype(np.float64)
    clean = 0.3 * gate * (np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 1760 * t))
    noisy = clean + 0.02 * np.random.default_rng(seed).standard_normal(n)
    return noisy.astype(np.float32), clean.astype(np.float32)


def reference(x, reduce_db=12.0):
    """X, P, lam (None where G = 1 by rule), G, y of the definition, float64 throughout"""
    x = np.asarray(x, np.float64)
    n = x.size
    T, lo, hi, _ = plan(n)
    xp = np.zeros((T - 1) * H + N)
    xp[N - H:N - H + n] = x
    w = np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))
    X = np.fft.rfft(np.stack([xp[m * H:m * H + N] * w for m in range(T)]), axis=1)
    P = np.abs(X) ** 2
    tot = np.zeros((T + 4, K + 2)); cnt = np.zeros((T + 4, K + 2))
    for dt in range(5):
        for dk in range(3):
            tot[dt:dt + T, dk:dk + K] += P; cnt[dt:dt + T, dk:dk + K] += 1
    S = (tot / np.maximum(cnt, 1))[2:T + 2, 1:K + 1]
    lam = None
    G = np.ones((T, K))
    if hi >= lo:
        M = np.empty((T, K))
        full = hi - lo >= 2 * D                     # else the window is every valid frame
        for m in range(T):
            a = max(lo, min(m - D, hi - 2 * D)) if full else lo
            b = a + 2 * D if full else hi
            M[m] = S[a:b + 1].min(axis=0)
        lam = C_BIAS * M
        xi = np.maximum(S / np.maximum(lam, 1e-30) - 1, 0)
        G = np.maximum(xi / (1 + xi), 10 ** (-reduce_db / 20))
    Y = np.fft.irfft(G * X, n=N, axis=1) * w
    y = np.zeros_like(xp)
    for m in range(T):
        y[m * H:m * H + N] += Y[m]
    return {"X": X, "P": P, "lam": lam, "G": G, "y": (y / 2)[N - H:N - H + n], "lo": lo, "hi": hi}


def noise_figures(r):
    """(noise_dbfs, snr_db) of q3_ref_audio_noise from a reference()'s lambda and P"""
    nz = max(r["lam"][r["lo"]:r["hi"] + 1].sum(axis=1).mean(), 1e-30)
    sig = max(r["P"][r["lo"]:r["hi"] + 1].sum(axis=1).mean() - nz, 1e-30)
    return 10 * np.log10(nz / 65536.0), 10 * np.log10(sig / nz)


def snr_db(y, clean):
    clean = np.asarray(clean, np.float64)
    return 10 * np.log10((clean ** 2).sum() / ((np.asarray(y, np.float64) - clean) ** 2).sum())
