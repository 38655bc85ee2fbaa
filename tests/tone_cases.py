"""What the tone tests share: the cookbook formulas, the band sets, the signal and the sequential cascades."""
import numpy as np

HP20 = [("hp", 20, 0.0, 0.707)]                                  # the worst pole radius
PEAK = [("peak", 3000, 24.0, 10.0)]
FULL = [("hp", 120), ("ls", 200, 4.0, 0.8), ("peak", 450, -6.0, 2.0), ("peak", 1000, 3.0, 1.0), ("peak", 3000, 6.0, 4.0),
        ("peak", 5200, -9.0, 6.0), ("hs", 8000, -2.0), ("lp", 10500, 0.0, 0.9)]
SETS = {"hp20": HP20, "peak": PEAK, "full": FULL}


def rbj(kind, f, db=0.0, q=0.707, rate=24000.0):
    """Audio EQ Cookbook: b0 b1 b2 a0 a1 a2 in float64"""
    A, w = 10.0 ** (db / 40.0), 2.0 * np.pi * f / rate
    c, al = np.cos(w), np.sin(w) / (2.0 * q)
    s = 2.0 * np.sqrt(A) * al
    return np.array({
        "peak": [1 + al * A, -2 * c, 1 - al * A, 1 + al / A, -2 * c, 1 - al / A],
        "ls": [A * ((A + 1) - (A - 1) * c + s), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - s),
               (A + 1) + (A - 1) * c + s, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - s],
        "hs": [A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s),
               (A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s],
        "hp": [(1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + al, -2 * c, 1 - al],
        "lp": [(1 - c) / 2, 1 - c, (1 - c) / 2, 1 + al, -2 * c, 1 - al]}[kind], np.float64)


def signal(n=9000):
    t = np.arange(n)
    x = 0.5 * np.random.default_rng(5).uniform(-1.0, 1.0, n) + 0.25 * np.sin(2.0 * np.pi * 55.0 * t / 24000.0)
    return x.astype(np.float32)


def cascade(x, bands, dtype=np.float64):
    """The sections one after the other, each a sequential transposed-direct-form-II recursion in `dtype` throughout."""
    y = np.asarray(x).astype(dtype)
    for band in bands:
        ba = rbj(*band)
        b0, b1, b2, a1, a2 = (dtype(v) for v in np.concatenate([ba[:3], ba[4:]]) / ba[3])
        s1 = s2 = dtype(0.0)
        out = np.empty_like(y)
        for i, v in enumerate(y):
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            out[i] = o
        y = out
    return y


def tolerance(ref64, ref32):
    """What the kernel may deviate from float64: twice the float32 recursion's own deviation, plus one f32 ulp of the peak."""
    return 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) + float(np.spacing(np.float32(np.abs(ref64).max())))
