"""Inputs, case tables and float64 references shared by tests/test_gpu_clone_ops.py (the kernels, -m gpu) and
tests/test_clone_ops_reference.py (what can be checked without a GPU). TEST INFRASTRUCTURE — no test lives here.

The voice-clone front end's own kernels: the speaker encoder's mel front end, reflect pad, column copy, SE scale + residual and the
attentive-statistics reductions (q3_speaker.hip), and the speech encoder's ELU, fold, codebook division and residual vector quantiser
(q3_mimi.hip). Tensors are [C][T], time contiguous. Every random input is seeded and read-only."""
import functools

import numpy as np

from codec_attn_cases import GUARD, SENT_BITS, is_sentinel, sentinel       # noqa: F401  (one sentinel for every op-level file)

CODE_SENT = np.uint32(0xA5A5A5A5)           # what `codes` holds going in: no codebook has that many entries


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def rel_dev(y, y64):
    """the measure of every bounded comparison but the mel: max |y - y64| / max |y64|"""
    y64 = np.asarray(y64, dtype=np.float64)
    return float(np.abs(np.asarray(y, dtype=np.float64) - y64).max() / np.abs(y64).max())


# ---------------------------------------------------------------- residual vector quantiser
def _rvq(proj, books, dtype):
    T = proj.shape[1]
    n_layers, CB, CD = books.shape
    r = np.ascontiguousarray(proj.T).astype(dtype)                       # [T][CD]
    bk = books.astype(dtype)
    codes = np.empty((T, n_layers), dtype=np.int64)
    resid = []
    for l in range(n_layers):
        resid.append(r.copy())
        d2 = np.zeros((T, CB), dtype=dtype)
        for d in range(CD):                                              # sequential over d, as the kernel and the oracle
            df = r[:, d, None] - bk[l, None, :, d]                       # rounded difference
            d2 = d2 + df * df                                            # rounded product, rounded running sum (numpy never fuses)
        win = np.argmin(d2, axis=1)                                      # first minimum
        codes[:, l] = win
        r = r - bk[l, win]
    return codes, resid


def rvq_f32(proj, books):
    """the kernel's arithmetic in numpy float32: proj [CD][T], books [n_layers][CB][CD] -> (codes [T][n_layers], the float32 residual
    [T][CD] entering each layer). Per layer d2 = sum_d (r[d] - e[d])^2 with the difference, the product and the running sum each rounded,
    np.argmin (first minimum), r -= e in float32."""
    return _rvq(proj, books, np.float32)


def rvq_f64(proj, books):
    return _rvq(proj, books, np.float64)


def rvq_naive(proj, books):
    """rvq_f32 as plain loops over frames, entries and dimensions — only to check the vectorised form on a tiny case"""
    T = proj.shape[1]
    n_layers, CB, CD = books.shape
    codes = np.empty((T, n_layers), dtype=np.int64)
    for t in range(T):
        r = [np.float32(proj[d, t]) for d in range(CD)]
        for l in range(n_layers):
            best, bidx = np.float32(np.inf), -1
            for e in range(CB):
                d2 = np.float32(0.0)
                for d in range(CD):
                    df = np.float32(r[d] - books[l, e, d])
                    d2 = np.float32(d2 + np.float32(df * df))
                if d2 < best:
                    best, bidx = d2, e
            codes[t, l] = bidx
            r = [np.float32(r[d] - books[l, bidx, d]) for d in range(CD)]
    return codes


# the "ties" case. 256 threads scan entries tid, tid + 256, ... in ascending order, then a tree over the threads (s = 128 ... 1) breaks
# equal distances by index. Integer values in [-2, 2]: every distance and every residual is exact in float32, so float32 and float64
# agree and nothing is a near-tie. CB = 600: threads 0..87 own three entries, the rest two.
TIES = dict(CD=8, CB=600, n_layers=3, T=8, n_q=5, q0=1)
# identical entries of layer 0, (lower, higher): the same thread (5 and 5 + 256); the two halves of the first reduction step (tid 10 /
# 138; tid 3 / 255); different strides of different threads (7 is tid 7's first entry, 300 tid 44's second). Frame i's input equals the
# pair's entry, so the tie is the minimum, at distance 0.
TIES_PAIRS = ((5, 261), (10, 138), (3, 255), (7, 300))
# the pair whose LOWER index sits in the HIGHER thread (200 is tid 200, 300 is tid 44): a reduction that preferred the lower thread
# would answer 300. Entry 300 of layer 0 is already entry 7's twin — a frame equal to it is won by 7 under either rule — so this pair
# is planted where nothing else can match: layer 1's entries 200 and 300 are its only zero vectors, and frame TIES_OWN_FRAME equals the
# unplanted layer-0 entry TIES_OWN_ENTRY exactly, so its residual entering layer 1 is zero. (The four pair frames leave layer 0 with a
# zero residual as well and meet the same tie.)
TIES_HIGH_THREAD = (200, 300)
TIES_OWN_FRAME, TIES_OWN_ENTRY = 4, 400


def _distinct_int_vectors(rng, n, dim, forbid_zero):
    seen, out = set(), []
    while len(out) < n:
        v = tuple(int(x) for x in rng.integers(-2, 3, size=dim))
        if v in seen or (forbid_zero and not any(v)):
            continue
        seen.add(v); out.append(v)
    return np.array(out, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def rvq_ties_case():
    """(proj [CD][T], books [n_layers][CB][CD]): frames 0..3 equal the TIES_PAIRS entries, frame TIES_OWN_FRAME the entry TIES_OWN_ENTRY,
    the rest are random integer vectors (their ties, where they occur, are between different entries at equal distance)"""
    c = TIES
    rng = np.random.default_rng(600)
    books = np.stack([_distinct_int_vectors(rng, c["CB"], c["CD"], forbid_zero=True) for _ in range(c["n_layers"])])
    for lo, hi in TIES_PAIRS:
        books[0, hi] = books[0, lo]
    books[1, list(TIES_HIGH_THREAD)] = 0.0
    proj = rng.integers(-2, 3, size=(c["CD"], c["T"])).astype(np.float32)
    for i, (lo, _) in enumerate(TIES_PAIRS):
        proj[:, i] = books[0, lo]
    proj[:, TIES_OWN_FRAME] = books[0, TIES_OWN_ENTRY]
    return _ro(proj, books)


# (name, CB, CD, n_layers, T): the tiny speech-encoder config's table (192 of 256 threads idle: their +inf / INT_MAX pass through the
# tree); two entries of one dimension (254 idle threads, tid >= CD from thread 1 on); CD one short of the 256-float residual with a
# second, ragged stride of entries (threads 0..43 own two)
RVQ_SMALL = (("tiny", 64, 24, 3, 5), ("two_entries", 2, 1, 2, 4), ("cd255", 300, 255, 2, 3))
# production: 2048 entries of 256 (eight per thread, every thread loads the residual), T = 3; the semantic group (one layer into column
# 0) and the acoustic group (15 layers into columns 1..15) write the same [T][16] codes, each from its own projection
RVQ_PROD = dict(CB=2048, CD=256, T=3, n_q=16, n_sem=1)


@functools.lru_cache(maxsize=None)
def rvq_float_case(name):
    """(proj, books) of standard-normal floats; name: an RVQ_SMALL name, "prod_sem" or "prod_ac" """
    if name.startswith("prod"):
        p = RVQ_PROD
        CB, CD, T = p["CB"], p["CD"], p["T"]
        n_layers = p["n_sem"] if name == "prod_sem" else p["n_q"] - p["n_sem"]
    else:
        _, CB, CD, n_layers, T = next(c for c in RVQ_SMALL if c[0] == name)
    rng = np.random.default_rng(sum(name.encode()) * 131 + CB)
    proj = rng.standard_normal((CD, T)).astype(np.float32)
    books = rng.standard_normal((n_layers, CB, CD)).astype(np.float32)
    return _ro(proj, books)


RVQ_FLOAT_NAMES = tuple(c[0] for c in RVQ_SMALL) + ("prod_sem", "prod_ac")


@functools.lru_cache(maxsize=None)
def rvq_expected(name):
    """(codes [T][n_layers], residuals) of rvq_f32 for "ties" or a float case — computed once"""
    proj, books = rvq_ties_case() if name == "ties" else rvq_float_case(name)
    codes, resid = rvq_f32(proj, books)
    codes.setflags(write=False)
    return codes, resid


# ---------------------------------------------------------------- mel front end
NF, HOP, PAD, NB = 1024, 256, 384, 513


def mel_frames(n):
    return (n + 2 * PAD - NF) // HOP + 1


def mel_index(n):
    """[T][1024] sample index of every frame position under the reference's clamped reflect rule (mel.rs:168-199): position p < 0 reads
    x[-p], or x[n - 1] when -p is beyond the clip; p >= n reads x[n - 2 - (p - n)], or x[0] when that is in front of it"""
    T = mel_frames(n)
    p = np.arange(T)[:, None] * HOP + np.arange(NF)[None, :] - PAD
    left = np.where(-p < n, -p, n - 1)
    i = p - n
    right = np.where(n >= 2 + i, n - 2 - i, 0)
    return np.where(p < 0, left, np.where(p >= n, right, p))


def _mel(x, win, fb, dtype):
    fr = x.astype(dtype)[mel_index(x.size)] * np.asarray(win).astype(dtype)      # [T][1024], the product rounded once in float32
    sp = np.fft.rfft(fr.astype(np.float64), axis=1)                              # the DFT is float64 in both forms, as the front end's
    re, im = sp.real.astype(dtype), sp.imag.astype(dtype)
    mag = np.sqrt(re * re + im * im + dtype(1e-9))
    mel = np.asarray(fb).astype(dtype) @ mag.T                                   # [n_mels][T]
    return np.log(np.maximum(mel, dtype(1e-5)))


def mel_ref64(x, win, fb):
    """the definition in float64 over the tables given: clamped reflect, window, 1024-point DFT, sqrt(re^2 + im^2 + 1e-9), fb @ mag,
    log(max(., 1e-5)) -> [n_mels][T]"""
    return _mel(np.asarray(x), win, fb, np.float64)


def mel_ref32(x, win, fb):
    """the same with every step but the DFT in numpy float32 (the front end computes its DFT in float64 by design): windowed samples,
    re / im, magnitude, filterbank sums and log are float32"""
    return _mel(np.asarray(x), win, fb, np.float32)


# white noise unless said. 256: T = 1 and both reflect clamps fire (-p reaches 384 > n - 1; p - n reaches 383 > n - 2); 300 / 384: the
# clamps fire for fewer positions, 384 is the last length at which the left one does; 385: the first length with neither; 640 / 1025:
# two / three frames, the right reflection crossing a hop; 5000: the shortest clip the whole-model test feeds. silence: every band at
# the 1e-5 floor. sine: full scale at bin 100 exactly — three live bins, leakage of nothing else, the other bands at the floor.
MEL_CASES = (("n256", 256), ("n300", 300), ("n384", 384), ("n385", 385), ("n640", 640), ("n1025", 1025), ("n5000", 5000),
             ("silence", 2048), ("sine", 2048))


@functools.lru_cache(maxsize=None)
def mel_case(name):
    n = dict(MEL_CASES)[name]
    if name == "silence":
        x = np.zeros(n, dtype=np.float32)
    elif name == "sine":
        x = np.sin(2.0 * np.pi * 100.0 * np.arange(n) / NF).astype(np.float32)          # 100 * 24000 / 1024 Hz at 24 kHz
    else:
        x = (0.25 * np.random.default_rng(n).standard_normal(n)).astype(np.float32)
    return _ro(x)


def hann64():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(NF) / NF))


def slaney_fb64(sr=24000, n_mels=128):
    """librosa's Slaney scale and area-normalised triangles in float64 (as tests/test_speaker_encoder.py::test_mel_filterbank_properties)"""
    def hz2mel(f):
        f = np.asarray(f, np.float64); return np.where(f < 1000, f / (200 / 3), 15 + np.log(np.maximum(f, 1e-9) / 1000) / (np.log(6.4) / 27))

    def mel2hz(m):
        m = np.asarray(m, np.float64); return np.where(m < 15, m * (200 / 3), 1000 * np.exp((m - 15) * (np.log(6.4) / 27)))
    pts = mel2hz(np.linspace(hz2mel(0.0), hz2mel(sr / 2.0), n_mels + 2))
    freqs = np.arange(NB) * sr / NF
    ref = np.zeros((n_mels, NB))
    for i in range(n_mels):
        lo, ce, up = pts[i], pts[i + 1], pts[i + 2]
        ref[i] = np.maximum(0, np.minimum((freqs - lo) / (ce - lo), (up - freqs) / (up - ce))) * 2 / (up - lo)
    return ref


def d_ref_mel(win, fb):
    """worst |mel_ref32 - mel_ref64| (absolute, on log-mel: log turns relative error into absolute) over MEL_CASES, on the tables given"""
    return max(float(np.abs(mel_ref32(mel_case(nm), win, fb).astype(np.float64) - mel_ref64(mel_case(nm), win, fb)).max()) for nm, _ in MEL_CASES)


# ---------------------------------------------------------------- speaker reductions
RED_C = 3
# 256 threads stride over time, then a four-wave tree: one element; two; one short of / exactly one wave; one short of / exactly / one
# past one element per thread; two strides and one element
RED_T = (1, 2, 63, 64, 255, 256, 257, 513)
CONST_VALUE = 0.75


@functools.lru_cache(maxsize=None)
def red_case(T):
    """x [3][T]: channel 0 standard normal; channel 1 constant (variance 0: std = sqrt(1e-5)); channel 2 = 1000 + 0.01 N(0, 1) (mean
    much larger than spread: (x - mean)^2 lives on the last bits of x)"""
    rng = np.random.default_rng(7000 + T)
    x = np.empty((RED_C, T), dtype=np.float32)
    x[0] = rng.standard_normal(T); x[1] = CONST_VALUE; x[2] = 1000.0 + 0.01 * rng.standard_normal(T)
    return _ro(x)


def mean_ref(x, dtype=np.float64):
    return x.astype(dtype).mean(axis=1, dtype=dtype)


def asp_in_ref(x, dtype=np.float64):
    """(x, mean [C], std [C]) with std = sqrt(mean((x - mean)^2) + 1e-5)"""
    x = x.astype(dtype)
    mean = x.mean(axis=1, dtype=dtype)
    d = x - mean[:, None]
    return x, mean, np.sqrt((d * d).mean(axis=1, dtype=dtype) + dtype(1e-5))


def asp_pool_ref(aw, m, dtype=np.float64):
    """(weighted mean [C], weighted std [C]): w = softmax over time of aw, mean = sum w m, std = sqrt(sum w (m - mean)^2 + 1e-5)"""
    aw = aw.astype(dtype); m = m.astype(dtype)
    w = np.exp(aw - aw.max(axis=1, keepdims=True)); w = w / w.sum(axis=1, keepdims=True, dtype=dtype)
    wm = (m * w).sum(axis=1, dtype=dtype)
    d = m - wm[:, None]
    return wm, np.sqrt((d * d * w).sum(axis=1, dtype=dtype) + dtype(1e-5))


def asp_pool_naive(aw, m):
    """asp_pool_ref as plain loops in float64 — only to check it on a tiny case"""
    C, T = aw.shape
    wm, ws = np.zeros(C), np.zeros(C)
    for c in range(C):
        mx = max(float(aw[c, t]) for t in range(T))
        e = [np.exp(float(aw[c, t]) - mx) for t in range(T)]
        s = sum(e)
        wm[c] = sum(float(m[c, t]) * e[t] / s for t in range(T))
        ws[c] = np.sqrt(sum((float(m[c, t]) - wm[c]) ** 2 * e[t] / s for t in range(T)) + 1e-5)
    return wm, ws


POOL_HOT_T, POOL_HOT_AT, POOL_HOT = 513, 300, 80.0
# (name, T): unit-normal-scale logits at every RED_T (T = 1: the softmax of one logit); "hot": one logit 80 above the rest at t = 300 of
# 513 (the second stride of thread 44: every other weight is below 1e-34, the pooled std is sqrt(1e-5)); "uniform": equal logits, the
# weighted mean is the plain mean; "deep": logits around -1e4 (only the subtraction of the maximum keeps exp from underflowing)
POOL_CASES = tuple(("normal", T) for T in RED_T) + (("hot", POOL_HOT_T), ("uniform", 513), ("deep", 257))


@functools.lru_cache(maxsize=None)
def pool_case(name, T):
    """(aw [3][T] logits, m [3][T] standard normal)"""
    rng = np.random.default_rng(8000 + T + 17 * len(name))
    m = rng.standard_normal((RED_C, T)).astype(np.float32)
    aw = (2.0 * rng.standard_normal((RED_C, T))).astype(np.float32)
    if name == "hot":
        aw[:, POOL_HOT_AT] = aw.max(axis=1) + np.float32(POOL_HOT)
    elif name == "uniform":
        aw[:] = np.float32(0.37)
    elif name == "deep":
        aw = (aw / 2.0 - 1.0e4).astype(np.float32)
    return _ro(aw, m)


def d_ref_reductions():
    """{op: worst rel_dev of the numpy-float32 restatement from float64 over this file's cases}; asp_in and asp_pool take the worst of
    their separately judged row groups"""
    d = {"mean": 0.0, "asp_in": 0.0, "asp_pool": 0.0, "elu": 0.0}
    for T in RED_T:
        x = red_case(T)
        d["mean"] = max(d["mean"], rel_dev(mean_ref(x, np.float32), mean_ref(x)))
        for y32, y64 in zip(asp_in_ref(x, np.float32), asp_in_ref(x)):
            d["asp_in"] = max(d["asp_in"], rel_dev(y32, y64))
    for name, T in POOL_CASES:
        aw, m = pool_case(name, T)
        for y32, y64 in zip(asp_pool_ref(aw, m, np.float32), asp_pool_ref(aw, m)):
            d["asp_pool"] = max(d["asp_pool"], rel_dev(y32, y64))
    for n in ELU_N:
        d["elu"] = max(d["elu"], rel_dev(elu_ref(elu_case(n), np.float32), elu_ref(elu_case(n))))
    for (L, r) in FOLD_PLAIN:
        x = fold_case(L)
        d["elu"] = max(d["elu"], rel_dev(fold_ref(x, r, fold_lf(L, r), elu=True, dtype=np.float32), fold_ref(x, r, fold_lf(L, r), elu=True)))
    return d


# ---------------------------------------------------------------- speaker movers (bit-exact)
MOVE_C = 3
# (T, pl, pr): the smallest legal T for one column each side; pads of (T - 1) / 2 and of T / 2; a pad across a 256-column block edge
# (Tp = 261: two blocks, the second with five live threads); tot == 0 — with b the Res2Net add alone, without b a plain copy through the
# kernel; an odd total pad (pl = tot / 2 rounds down: the right side is the longer one)
PAD_CASES = ((2, 1, 1), (5, 2, 2), (9, 4, 4), (257, 2, 2), (300, 0, 0), (6, 1, 2))
SE_T = (1, 256, 257)


@functools.lru_cache(maxsize=None)
def pad_case(T, pl, pr):
    """(a [3][T], b [3][T], src [3][T + pl + pr] for the column copy)"""
    rng = np.random.default_rng(T * 100 + pl * 10 + pr)
    a, b = (rng.standard_normal((MOVE_C, T)).astype(np.float32) for _ in range(2))
    src = rng.standard_normal((MOVE_C, T + pl + pr)).astype(np.float32)
    return _ro(a, b, src)


def pad_ref(a, b, pl, pr):
    """reflect padding without the edge sample repeated (speaker.rs:24-51) of a (+ b, one rounded float32 add)"""
    v = a if b is None else a + b
    return np.pad(v, ((0, 0), (pl, pr)), mode="reflect") if pl + pr else v.copy()


@functools.lru_cache(maxsize=None)
def se_case(T):
    rng = np.random.default_rng(9000 + T)
    o, h = (rng.standard_normal((MOVE_C, T)).astype(np.float32) for _ in range(2))
    g = rng.uniform(0.0, 1.0, MOVE_C).astype(np.float32)                 # a sigmoid's range
    return _ro(o, g, h)


def se_ref(o, g, h):
    return (o * g[:, None]) + h                                          # float32: one rounded multiply, one rounded add


# ---------------------------------------------------------------- speech-encoder movers
FOLD_C = 2
# plain mode (L, r), Lf = ceil(L / r): one sample into two phases (phase 1 is all fill); L not a multiple of r with 2 / 1 / 5 zero-filled
# tail samples; exact multiples (no fill); 513 / 2: a second 256-column block with one live thread, one fill sample
FOLD_PLAIN = ((1, 2), (7, 3), (8, 4), (11, 5), (13, 6), (16, 8), (513, 2))
# replicate mode, r = 2, (L, Lf): one sample (column 0, the sample and its repeat are all x[0]); an exact fit (no repeat); one repeat of
# x[L - 1]; the same across a block edge (W = 257)
FOLD_REPL = ((1, 1), (6, 3), (7, 4), (511, 256))


def fold_lf(L, r):
    return -(-L // r)


@functools.lru_cache(maxsize=None)
def fold_case(L):
    return _ro((2.0 * np.random.default_rng(300 + L).standard_normal((FOLD_C, L))).astype(np.float32))


def elu_ref(x, dtype=np.float64):
    x = x.astype(dtype)
    return np.where(x > 0, x, np.expm1(x) if dtype is np.float64 else np.exp(np.minimum(x, dtype(0))) - dtype(1))


def fold_ref(x, r, Lf, elu=False, replicate=False, dtype=np.float32):
    """y [C*r][Lf + lead]: row c*r + p, column lead + tau = f(x[c][tau*r + p]); beyond L zeros (plain) or x[c][L - 1] (replicate, whose
    leading column is x[c][0] for every phase). f = ELU in `dtype` or the identity."""
    C, L = x.shape
    xp = np.pad(x, ((0, 0), (0, Lf * r - L)), mode="edge" if replicate else "constant") if Lf * r > L else x[:, :Lf * r]
    y = xp.reshape(C, Lf, r).transpose(0, 2, 1).reshape(C * r, Lf)
    if replicate:
        y = np.concatenate([np.repeat(x[:, :1], r, axis=0), y], axis=1)
    return elu_ref(y, dtype) if elu else y.astype(dtype)


def fold_naive(x, r, Lf, replicate=False):
    """fold_ref (identity) as plain loops — only to check it on tiny cases"""
    C, L = x.shape
    lead = 1 if replicate else 0
    y = np.zeros((C * r, Lf + lead), dtype=x.dtype)
    for c in range(C):
        for p in range(r):
            if replicate:
                y[c * r + p, 0] = x[c, 0]
            for tau in range(Lf):
                i = tau * r + p
                y[c * r + p, lead + tau] = x[c, i] if i < L else (x[c, L - 1] if replicate else 0.0)
    return y


ELU_N = (1, 255, 256, 257)                  # 256 elements per workgroup


@functools.lru_cache(maxsize=None)
def elu_case(n):
    """N(0, 2) with 0.0 and -1e-6 planted (n > 2): exp(x) - 1 loses every digit of a tiny x; n = 1: one negative value"""
    x = (2.0 * np.random.default_rng(500 + n).standard_normal(n)).astype(np.float32)
    if n > 2:
        x[1] = 0.0; x[2] = -1.0e-6
    else:
        x[0] = -abs(x[0])
    return _ro(x)


CODEBOOK_USAGE = (0.0, 1.0e-6, 1.0e-5, 0.5, 3.0, 1.0e4)      # below / at / above the 1e-5 clamp
CODEBOOK_DIMS = (24, 256, 300)              # the tiny config's dim; one stride of 256 threads; a second, ragged one


@functools.lru_cache(maxsize=None)
def codebook_case(dim):
    """(embed_sum [6][dim], cluster_usage [6], expected [6][dim] = esum / max(usage, 1e-5) in numpy float32)"""
    esum = (3.0 * np.random.default_rng(dim).standard_normal((len(CODEBOOK_USAGE), dim))).astype(np.float32)
    usage = np.array(CODEBOOK_USAGE, dtype=np.float32)
    exp = esum / np.maximum(usage, np.float32(1e-5))[:, None]
    return _ro(esum, usage, exp)


def ulp_diff(a, b):
    """largest distance between two float32 arrays in units in the last place (finite values)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


# ---------------------------------------------------------------- D_REF
# What the same formulas in numpy float32 deviate from float64 over the cases of this file (d_ref_mel on the encoder's own tables,
# d_ref_reductions), measured on the CPU; each constant lies about 18 % above its measurement, the play a float32 library has between
# CPUs. test_clone_ops_reference.py recomputes them and holds each measurement to [0.5, 1.0] x its constant. The GPU bound is 4 x the
# constant (test_gpu_attention_op.py's rule: two for another summation order, two for a fast exp).
D_REF_MEL = 1.18e-6          # measured 1.00e-6 (the sine case; white noise 1.7e-7 .. 3.0e-7, silence 3.2e-7), absolute on log-mel
D_REF_MEAN = 7.0e-8          # measured 5.91e-8
D_REF_ASP_IN = 1.65e-7       # measured 1.40e-7
D_REF_ASP_POOL = 2.73e-7     # measured 2.31e-7
D_REF_ELU = 2.0e-8           # measured 1.70e-8 (k_mimi_elu's cases and the plain folds with ELU on)
