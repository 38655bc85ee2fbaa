"""The output stage's loudness step, host side: the K-weighting against the tables printed in ITU-R BS.1770-4 and
against the fixture, the constants, the refusals — and the definition restated in numpy float32, every operation rounded once and
every sum in the stage's order, which must reproduce the float64 fixture (tests/make_golden_loudness.py, scipy at generation time
only). The `gpu` tests of test_loudness_stage.py import the restatement and hold the device to it BITWISE. No GPU here."""
import ctypes
import functools
import os

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api

NEW = ["q3_loudness_kweight", "q3_pcm_stage_loudness_consts", "q3_pcm_stage_set_loudness", "q3_pcm_stage_loudness",
       "q3_pcm_stage_loudness_blocks", "q3_session_set_loudness", "q3_session_loudness", "q3_batcher_ticket_loudness",
       "q3_batcher_ticket_loudness_read"]
FS, HOP, HIST = 24000, 2400, 4096
Q3_INVALID_ARG = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loudness_kats.npz")
f32, f64 = np.float32, np.float64
# the f32-against-f64 gap measured with this restatement is at most 6.8e-6 LU (integrated) and 1.8e-6 relative (gated block
# values: those that pass both gates); the allowance is ten times the largest measured, rounded up
TOL_LU, TOL_REL = 1e-4, 2e-5

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2
BS1770_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
BS1770_HIGHPASS = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


# ---------------------------------------------------------------- the signals, from seeds
SIGNALS = {
    "sine": dict(kind="sine", seconds=5.0, seed=0),
    "gated_noise": dict(kind="gated_noise", seconds=4.0, seed=11),
    "steps": dict(kind="steps", seconds=10.0, seed=0),
    "speech_like": dict(kind="speech_like", seconds=5.0, seed=23),
}


def make_signal(name):
    """float32, 24 kHz; built in float64 from the seed and rounded once"""
    p = SIGNALS[name]
    n = int(round(p["seconds"] * FS))
    t = np.arange(n, dtype=f64) / FS
    rng = np.random.default_rng(p["seed"])
    if p["kind"] == "sine":                                # 997 Hz, full scale
        x = np.sin(2.0 * np.pi * 997.0 * t)
    elif p["kind"] == "gated_noise":                       # Gaussian noise in half-second stretches: on, 60 dB down, on, silent, ...
        amp = np.array([0.1, 0.0001, 0.1, 0.0, 0.05, 0.1, 0.002, 0.1])
        x = rng.standard_normal(n) * np.repeat(amp, n // amp.size)
    elif p["kind"] == "steps":                             # 997 Hz at -46 / -23 / -46 dBFS for 2 / 6 / 2 s
        a = np.where((t >= 2.0) & (t < 8.0), 10.0 ** (-23.0 / 20.0), 10.0 ** (-46.0 / 20.0))
        x = a * np.sin(2.0 * np.pi * 997.0 * t)
    else:                                                  # noise under a syllabic envelope (4 Hz) with pauses
        env = np.maximum(0.0, np.sin(2.0 * np.pi * 4.0 * t)) ** 2 * (np.sin(2.0 * np.pi * 0.35 * t + 0.4) > -0.5)
        x = 0.12 * env * rng.standard_normal(n)
    return x.astype(f32)


# ---------------------------------------------------------------- the definition, restated
def kweight_np(fs):
    """(shelf, high-pass), each b0 b1 b2 a0 a1 a2 in float64: BS.1770's prototypes through the tangent pre-warped bilinear form"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs); Vh = 10.0 ** (G / 20.0); Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    sh = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(sh, f64), np.array(hp, f64)


def consts_np(target_mb=-1900, prior_mb=0):
    """T, P, gate_abs, a_lo, a_hi: float64, rounded once"""
    return (f32(10.0 ** ((target_mb / 100.0 + 0.691) / 10.0)), f32(10.0 ** (prior_mb / 2000.0)), f32(10.0 ** ((-70.0 + 0.691) / 10.0)),
            f32(10.0 ** (-2400.0 / 2000.0)), f32(10.0 ** (2400.0 / 2000.0)))


def _biquad(V, ba):
    """transposed direct form II down the rows of V [n, lanes] (the lanes are independent streams), float32, each operation
    rounded once:  o = b0 v + s1;  s1 = (b1 v - a1 o) + s2;  s2 = b2 v - a2 o"""
    b0, b1, b2, _, a1, a2 = [f32(c) for c in ba]
    P0, P1, P2 = b0 * V, b1 * V, b2 * V                     # (products of the input: no recursion in them)
    O = np.empty_like(V)
    s1 = np.zeros(V.shape[1], f32); s2 = np.zeros(V.shape[1], f32)
    for i in range(V.shape[0]):
        o = P0[i] + s1
        s1 = (P1[i] - a1 * o) + s2
        s2 = P2[i] - a2 * o
        O[i] = o
    assert O.dtype == np.float32
    return O


def _fold64(S):
    """S [.., 64] -> [..]: for d = 32 .. 1, s_q = s_q + s_(q+d) for q < d"""
    S = S.copy()
    d = 32
    while d >= 1:
        S[..., :d] = S[..., :d] + S[..., d:2 * d]
        d //= 2
    return S[..., 0]


def _sum64(v, dtype):
    """the sum of v in 64 interleaved partials (index mod 64, ascending), folded"""
    m = (v.size + 63) // 64
    a = np.zeros(m * 64, dtype); a[:v.size] = v             # (+0.0 leaves a sum of non-negative terms as it is)
    a = a.reshape(m, 64)
    s = np.zeros(64, dtype)
    for r in range(m):
        s = s + a[r]
    return _fold64(s)


def k_energies(X):
    """hop energies e [lanes, hops] (float32) of the streams X [lanes, n]: K-weighting (a non-finite sample enters as 0), squares
    in 64 interleaved partial sums per hop"""
    X = np.asarray(X, f32)
    sh, hp = kweight_np(FS)
    V = np.where(np.isfinite(X), X, f32(0.0)).T.copy()
    K = _biquad(_biquad(V, sh), hp)
    hops = X.shape[1] // HOP
    K2 = (K * K)[:hops * HOP].T.reshape(X.shape[0], hops, HOP)
    pad = np.zeros((X.shape[0], hops, 38 * 64), f32); pad[:, :, :HOP] = K2
    pad = pad.reshape(X.shape[0], hops, 38, 64)
    s = np.zeros((X.shape[0], hops, 64), f32)
    for r in range(38):
        s = s + pad[:, :, r, :]
    e = _fold64(s)
    assert e.dtype == np.float32
    return e


def blocks_of(e):
    """z_3 .. of one stream's hop energies"""
    e = np.asarray(e, f32)
    if e.size < 4:
        return np.zeros(0, f32)
    return ((e[:-3] + e[1:-2]) + (e[2:-1] + e[3:])) * f32(1.0 / 9600.0)


def gate(z, gate_abs):
    """(M, cg) over the block values z, or None without an estimate: float64 sums in 64 interleaved partials"""
    z = np.asarray(z, f32)
    above = z > gate_abs
    ca = int(above.sum())
    if ca == 0:
        return None
    Sa = _sum64(np.where(above, z.astype(f64), 0.0), f64)
    Gr = 0.1 * Sa / ca
    keep = above & (z.astype(f64) > Gr)
    cg = int(keep.sum())
    Sg = _sum64(np.where(keep, z.astype(f64), 0.0), f64)
    return f32(Sg / cg), cg


def track(e, target_mb=-1900, prior_mb=0):
    """the row after every hop of e: (z stored, M per hop, A per hop, cg after the last) — M is 0 until there is an estimate, and
    M and A are frozen past HIST blocks"""
    T, P, ga, lo, hi = consts_np(target_mb, prior_mb)
    z = blocks_of(e)[:HIST]
    Ms = np.zeros(len(e), f32); As = np.zeros(len(e), f32)
    M = f32(0.0); A = P; cg = 0
    for h in range(len(e)):
        if h < 3:
            A = P
        elif h - 3 < HIST:
            g = gate(z[:h - 2], ga)
            if g is not None:
                M, cg = g
                A = min(max(np.sqrt(T / M), lo), hi)
                assert type(A) is np.float32
        Ms[h] = M; As[h] = A
    return z, Ms, As, cg


def normalise(x, As, prior_mb=0):
    """y = x G: sample j of hop h under g0 + (g1 - g0) (j / 2400), g0 = A_(h-2), g1 = A_(h-1) (P before the first hop)"""
    x = np.asarray(x, f32)
    P = consts_np(-1900, prior_mb)[1]
    hops = (x.size + HOP - 1) // HOP
    Ap = np.concatenate([np.full(2, P, f32), np.asarray(As, f32)])         # Ap[h + 2] = A_h
    h = np.arange(x.size) // HOP
    g0 = Ap[h]; g1 = Ap[h + 1]
    assert hops <= len(As) + 1
    frac = (np.arange(x.size) % HOP).astype(f32) / f32(HOP)
    G = g0 + (g1 - g0) * frac
    y = x * G
    assert y.dtype == np.float32
    return y


def lufs(M):
    return -0.691 + 10.0 * np.log10(float(M)) if float(M) > 0.0 else float("-inf")


@functools.lru_cache(maxsize=None)
def reference():
    """{name: (x, e, z, M per hop, A per hop at -1900 / 0, cg)} of the four signals: one pass of the recursion with the signals as
    lanes, computed once per process and shared (read-only) by every test that needs it"""
    xs = {n: make_signal(n) for n in SIGNALS}
    L = max(x.size for x in xs.values())
    X = np.zeros((len(xs), L), f32)
    for i, x in enumerate(xs.values()):
        X[i, :x.size] = x
    E = k_energies(X)
    out = {}
    for i, (n, x) in enumerate(xs.items()):
        e = E[i, :x.size // HOP].copy()
        z, Ms, As, cg = track(e)
        for a in (x, e, z, Ms, As):
            a.setflags(write=False)
        out[n] = (x, e, z, Ms, As, cg)
    return out


# ---------------------------------------------------------------- tests
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert callable(api.PcmStage.set_loudness) and callable(api.PcmStage.loudness) and callable(api.PcmStage.loudness_blocks)
    assert callable(api.Session.set_loudness) and callable(api.Session.loudness) and callable(api.Batcher.loudness) and callable(api.loudness)
    assert (api.LOUD_OFF, api.LOUD_METER, api.LOUD_NORMALIZE) == (0, 1, 2)


def test_kweight_48k_is_the_table_of_bs1770():
    sh, hp = api.loudness_kweight(48000)
    for got, want in ((sh, BS1770_SHELF), (hp, BS1770_HIGHPASS)):
        assert got[3] == 1.0
        np.testing.assert_allclose(got[[0, 1, 2, 4, 5]], want, rtol=0, atol=1e-12)
    nsh, nhp = kweight_np(48000)
    np.testing.assert_allclose(nsh[[0, 1, 2, 4, 5]], BS1770_SHELF, rtol=0, atol=1e-12)
    np.testing.assert_allclose(nhp[[0, 1, 2, 4, 5]], BS1770_HIGHPASS, rtol=0, atol=1e-12)


def test_kweight_24k_is_the_fixture():
    g = np.load(GOLDEN)
    sh, hp = api.loudness_kweight(24000)
    np.testing.assert_allclose(sh, g["shelf_24k"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(hp, g["highpass_24k"], rtol=0, atol=1e-15)
    for fs in (8000, 16000, 44100, 96000, 192000):
        a, b = api.loudness_kweight(fs); c, d = kweight_np(fs)
        np.testing.assert_allclose(a, c, rtol=0, atol=1e-14); np.testing.assert_allclose(b, d, rtol=0, atol=1e-14)


def test_consts_to_one_ulp_of_numpy():
    for target in list(range(-4000, -499, 53)) + [-500, -1900, -2300, -1600]:
        for prior in (-6000, -1234, -1, 0, 600, 2400):
            got = api.pcm_stage_loudness_consts(target, prior)
            for g, w in zip(got, consts_np(target, prior)):
                assert abs(float(g) - float(w)) <= float(np.spacing(w)), (target, prior, g, w)
    T, P, ga, lo, hi = api.pcm_stage_loudness_consts(-1900, 0)
    assert P == f32(1.0) and abs(lufs(T) - (-19.0)) < 1e-6 and abs(lufs(ga) - (-70.0)) < 1e-5
    assert abs(20.0 * np.log10(float(hi)) - 24.0) < 1e-6 and abs(20.0 * np.log10(float(lo)) + 24.0) < 1e-6


def test_range_errors_of_the_host_functions():
    L = _lib.lib
    sh = (ctypes.c_double * 6)(); hp = (ctypes.c_double * 6)(); v = ctypes.c_float()
    for fs in (0, 7999, 192001, 1 << 31):
        assert L.q3_loudness_kweight(fs, sh, hp) == Q3_INVALID_ARG and len(L.q3_last_error()) > 0
    assert L.q3_loudness_kweight(48000, None, hp) == Q3_INVALID_ARG and L.q3_loudness_kweight(48000, sh, None) == Q3_INVALID_ARG
    for fs in (8000, 192000):
        assert L.q3_loudness_kweight(fs, sh, hp) == 0
    for target, prior in ((-4001, 0), (-499, 0), (0, 0), (-1900, -6001), (-1900, 2401), (1900, 0)):
        assert L.q3_pcm_stage_loudness_consts(target, prior, ctypes.byref(v), None, None, None, None) == Q3_INVALID_ARG
        assert len(L.q3_last_error()) > 0
        with pytest.raises(_lib.Q3Error):
            api.pcm_stage_loudness_consts(target, prior)
    for target, prior in ((-4000, -6000), (-500, 2400)):
        assert L.q3_pcm_stage_loudness_consts(target, prior, None, None, None, None, None) == 0


def test_null_handles_give_a_status_and_a_message():
    L = _lib.lib
    n = ctypes.c_size_t()
    for f in (lambda: L.q3_pcm_stage_set_loudness(None, 0, 2, -1900, 0), lambda: L.q3_pcm_stage_loudness(None, 0, None, None, None, None),
              lambda: L.q3_pcm_stage_loudness_blocks(None, 0, None, 0, ctypes.byref(n)), lambda: L.q3_session_set_loudness(None, 0, 2, -1900, 0),
              lambda: L.q3_session_loudness(None, 0, None, None, None, None), lambda: L.q3_batcher_ticket_loudness(None, 1, 2, -1900, 0),
              lambda: L.q3_batcher_ticket_loudness_read(None, 1, None, None, None, None)):
        assert f() == Q3_INVALID_ARG and len(L.q3_last_error()) > 0


def test_restatement_reproduces_the_fixture():
    """float32 in the stage's order against float64 through scipy.signal.lfilter: hop energies and gated block values within 2e-5
    relative, integrated loudness within 1e-4 LU; the 997 Hz sine reads -3.01 LKFS within EBU Tech 3341's +-0.1 LU."""
    g = np.load(GOLDEN)
    assert [str(n) for n in g["names"]] == list(SIGNALS)
    ref = reference()
    ga = consts_np()[2]
    for name in SIGNALS:
        p = SIGNALS[name]
        assert int(g[name + "_seed"]) == p["seed"] and int(g[name + "_n"]) == int(round(p["seconds"] * FS))
        x, e, z, Ms, As, cg = ref[name]
        ge, gz, gl = g[name + "_e"], g[name + "_z"], float(g[name + "_lufs"])
        assert e.size == ge.size and z.size == gz.size == e.size - 3
        keep = gz > float(ga)
        keep &= gz > 0.1 * gz[keep].mean()                 # the gated blocks: those that pass both gates in float64
        rel = np.abs(z[keep].astype(f64) - gz[keep]) / gz[keep]
        gap = abs(lufs(Ms[-1]) - gl)
        print(f"{name}: {z.size} blocks, {cg} gated; gated block values within {rel.max():.2e} relative, "
              f"integrated {lufs(Ms[-1]):.6f} LUFS against {gl:.6f}: gap {gap:.2e} LU")
        assert cg == int(g[name + "_gated"]) == int(keep.sum())
        assert rel.max() <= TOL_REL, (name, rel.max())
        assert gap <= TOL_LU, (name, gap)
    assert abs(float(g["sine_lufs"]) - (-2.984)) < 1e-3
    assert abs(lufs(ref["sine"][3][-1]) - (-3.01)) <= 0.1


def test_restatement_tracks_as_defined():
    """the first three hops at the prior, the first estimate after the fourth; silence keeps the prior; a gain never leaves
    +-24 dB; the normalised steps signal ends near the target"""
    x, e, z, Ms, As, cg = reference()["steps"]
    T, P, ga, lo, hi = consts_np()
    assert np.all(As[:3] == P) and Ms[2] == 0 and Ms[3] > 0 and As[3] != P
    assert np.all(As >= lo) and np.all(As <= hi)
    assert As[3] == hi                                     # -46 dBFS to -19 LUFS asks for more than +24 dB
    ze, zM, zA, zc = track(np.zeros(20, f32), prior_mb=-600)[0:4]
    assert np.all(zA == consts_np(-1900, -600)[1]) and np.all(zM == 0) and zc == 0
    y = normalise(x, As)
    assert np.array_equal(y[:HOP * 4], x[:HOP * 4])         # 400 ms at the prior (1.0)
    assert not np.array_equal(y[HOP * 4:HOP * 5], x[HOP * 4:HOP * 5])
    assert abs(20.0 * np.log10(float(As[-1])) - (-19.0 - lufs(Ms[-1]))) < 1e-4
