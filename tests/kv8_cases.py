"""Plain reference of the KV8 cache format and the case tables of tests/test_gpu_kv8.py.

Rule (the FP8 weights' of DESIGN 4.1a, per cached row of 128 elements): e = the smallest integer with amax * 2^-e <= 448, 0 for
an all-zero row, never below -120; code = RNE_e4m3(x * 2^-e); the scale is stored as the E8M0 byte e + 127."""
import numpy as np
import torch

from attn_step_cases import K, RATIOS

EMIN = -120
POS = (0, 1, 7, 8, 31, 32, 33, 95, 96, 97, 127, 128, 129)      # the 8-position wave step, the 32-position round, the three-deep rotation, the page edge
POS_ROWS = [(0, 1, 7), (8, 31, 32), (33, 95, 96), (97, 127, 128), (129, 5, 64)]      # B = 3 with unequal positions; together: POS
assert set(POS) <= {p for r in POS_ROWS for p in r}
SPLITS = (1, 3, 8)              # with 1 .. 130 keys: splits with an empty range included
STEP_KEYS = [K(nh, nkv, 256, pos) for nh, nkv in RATIOS for pos in POS_ROWS]
DEEP_KEY = K(4, 2, 9 * 128, (8 * 128 + 5,))                    # page 8 of a row: only the one-entry-per-lane table form names it
SLICE_KEY = K(4, 2, 256, (33, 128, 200), kind="slices", S=2)
ZERO_KEY = K(4, 2, 256, (3, 130, 255))


def exponent(amax):
    """amax = f * 2^x with f in [0.5, 1): amax * 2^-e <= 448 = 0.875 * 2^9 <=> e >= x - 9, one more where f > 0.875"""
    amax = np.asarray(amax, dtype=np.float64)
    f, x = np.frexp(amax)
    e = x - 9 + (f > 0.875)
    return np.where(amax > 0, np.maximum(e, EMIN), 0).astype(np.int32)


def quantize_rows(x):
    """x [..., 128] -> (codes u8 [..., 128], scale bytes u8 [...], dequantised f64 [..., 128])"""
    x = np.asarray(x, dtype=np.float64)
    e = exponent(np.abs(x).max(axis=-1))
    scale = np.exp2(e.astype(np.float64))[..., None]
    f8 = torch.from_numpy(np.ascontiguousarray(x / scale)).to(torch.float8_e4m3fn)          # exact quotient, RNE
    return f8.view(torch.uint8).numpy(), (e + 127).astype(np.uint8), f8.to(torch.float64).numpy() * scale


def dequantize(codes, scales):
    f8 = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint8)).view(torch.float8_e4m3fn)
    return f8.to(torch.float64).numpy() * np.exp2(np.asarray(scales, dtype=np.float64) - 127.0)[..., None]


def e4m3_step(c):
    """spacing of e4m3 numbers at |c| (c in code units, |c| <= 448): 2^-9 below 2^-6, else 2^(floor(log2 |c|) - 3)"""
    _, x = np.frexp(np.maximum(np.abs(np.asarray(c, dtype=np.float64)), 2.0 ** -6))
    return np.exp2(x - 1 - 3.0)


def converter_pages(seed=5):
    """src [3 pages][2 layers][K, V][2 kv heads][128][128] f32: rows scaled by powers of two over 60 binades, and the rows the rule has
    edges at — all zero, one huge element, amax below 448 * 2^-120, amax on and next to the 0.875 / 1.0 mantissa boundaries"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((3, 2, 2, 2, 128, 128)) * np.exp2(rng.integers(-30, 30, (3, 2, 2, 2, 128, 1)).astype(np.float64))
    src = src.astype(np.float32)
    rows = src.reshape(-1, 128)
    at = iter(rng.permutation(rows.shape[0])[:64])
    rows[next(at)] = 0.0
    r = next(at); rows[r] *= 2.0 ** -40; rows[r, 77] = np.float32(-1.5 * 2.0 ** 100)
    rows[next(at)] = (rng.standard_normal(128) * 2.0 ** -128).astype(np.float32)
    for k in (-20, 0, 9, 31):
        for amax in (0.875, np.nextafter(np.float32(0.875), np.float32(1)), np.nextafter(np.float32(0.875), np.float32(0)), 1.0,
                     np.nextafter(np.float32(1), np.float32(0))):
            r = next(at)
            rows[r] = (rng.uniform(-0.5, 0.5, 128) * 2.0 ** k).astype(np.float32)
            rows[r, int(rng.integers(128))] = np.float32(-amax) * np.float32(2.0 ** k)
    return src
