"""Op-level tests of the voice-clone encoders' own kernels (-m gpu): one launch at a time against numpy. Inputs, case tables (each
names what it reaches) and references live in clone_ops_cases.py; what needs no GPU — the references against plain loops, the tie
case's own claims, the D_REF recomputation, the refusal of bad shapes — is in test_clone_ops_reference.py.

k_mimi_rvq (q3_mimi_rvq_ex -> ONE launch_mimi_rvq): the codes equal rvq_f32 — the kernel's distance arithmetic in numpy float32, first
minimum — exactly on every case, exact ties included; `codes` goes in filled with a sentinel word and every column outside
[q0, q0 + n_layers) keeps it.
k_spk_stft_mel (SpeakerEncoder.mel, one launch): finite, of shape (128, mel_frames(n)), within 4 x D_REF_MEL (absolute, on log-mel) of
the float64 definition over the encoder's own tables, which are read back and held to float64 Hann / Slaney references and to the
oracle's tables.
k_spk_mean / k_spk_asp_in / k_spk_asp_pool / k_mimi_elu and the fold with ELU on: max |y - y64| / max |y64| per case and per output
row group, bound 4 x the op's D_REF (what the same formula in numpy float32 deviates from float64 over the same cases; two for another
summation order, two for a fast exp).
k_spk_pad / k_spk_cols / k_spk_se_apply / k_mimi_fold without ELU: bit-equal to numpy float32; so is k_mimi_codebook (the bound
asked for is 1 ulp; it measured 0 ulp at every dim, so bit-equality is asserted as well).
Every destination is a NaN of known bits with guard elements on both sides: what a launch owns must be finite, the rest must keep
those bits.

Measured on an MI355X (worst over every case of this file, in units of the op's D_REF; bound 4; each test prints its own with -s):
  k_spk_stft_mel 1.35 (the sine and the silence case, 1.59e-6 on log-mel; white noise 0.28 .. 0.48), k_spk_mean 0.94,
  k_spk_asp_in mean 0.40 / std 1.11, k_spk_asp_pool mean 0.70 / std 0.33, k_mimi_elu 0.85, k_mimi_fold with ELU 0.91
  window 1.63 ulp(1) from the float64 Hann (bound 2); filterbank 6.1e-7 from the float64 Slaney table (0.008 of its bound) and
  bit-equal to the oracle's, as is the window; k_mimi_codebook 0 ulp; k_mimi_rvq equal to rvq_f32 on every case
No kernel missed a check."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import clone_ops_cases as C
import oracle as O
from clone_ops_cases import GUARD
from qwen3_tts_rs_amd.api import (SPK_PAD, SPK_COLS, SPK_MEAN, SPK_SE_APPLY, SPK_ASP_IN, SPK_ASP_POOL, MIMI_ELU, MIMI_FOLD, MIMI_CODEBOOK)

pytestmark = pytest.mark.gpu

WORST = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and (_bits(a) == _bits(b)).all()


def _record(name, dev, d_ref):
    WORST[name] = max(WORST.get(name, 0.0), dev / d_ref)
    print(f"{name}: dev {dev:.3e} = {dev / d_ref:.2f} D_REF; worst so far {({k: round(v, 2) for k, v in WORST.items()})}")


def _guarded(n):
    """(buffer, payload slice): n result floats between two guards, all sentinel"""
    return C.sentinel(GUARD + n + GUARD), slice(GUARD, GUARD + n)


def _guards_kept(buf, n):
    return C.is_sentinel(buf[:GUARD]).all() and C.is_sentinel(buf[GUARD + n:]).all()


# ---------------------------------------------------------------- residual vector quantiser
def _rvq_run(name, n_q, q0, codes=None):
    proj, books = C.rvq_ties_case() if name == "ties" else C.rvq_float_case(name)
    if codes is None:
        codes = np.full((proj.shape[1], n_q), C.CODE_SENT, dtype=np.uint32)
    return q.mimi_rvq_ex(proj, books, codes, q0=q0)


def _rvq_check(codes, name, q0):
    want, _ = C.rvq_expected(name)
    nl = want.shape[1]
    got = codes[:, q0:q0 + nl].astype(np.int64)
    assert (got == want).all(), f"{name}: frames x layers that differ from rvq_f32: {np.argwhere(got != want).tolist()} got {got[got != want].tolist()} want {want[got != want].tolist()}"


def test_rvq_ties():
    """identical entries in one thread, across the halves of the first reduction step, in different strides, and the pair whose lower
    index sits in the higher thread: the lower index wins every time"""
    c = C.TIES
    codes = _rvq_run("ties", c["n_q"], c["q0"])
    _rvq_check(codes, "ties", c["q0"])
    for i, (lo, _) in enumerate(C.TIES_PAIRS):
        assert codes[i, c["q0"]] == lo
    assert codes[C.TIES_OWN_FRAME, c["q0"] + 1] == C.TIES_HIGH_THREAD[0]
    assert (codes[:, :c["q0"]] == C.CODE_SENT).all() and (codes[:, c["q0"] + c["n_layers"]:] == C.CODE_SENT).all()


@pytest.mark.parametrize("name,CB,CD,n_layers,T", C.RVQ_SMALL)
def test_rvq_small(name, CB, CD, n_layers, T):
    codes = _rvq_run(name, n_layers + 2, 1)
    _rvq_check(codes, name, 1)
    assert (codes[:, 0] == C.CODE_SENT).all() and (codes[:, -1] == C.CODE_SENT).all()


def test_rvq_production_groups():
    """2048 x 256: the semantic group writes column 0 and leaves the rest, the acoustic group writes columns 1..15 of the same buffer
    and leaves column 0"""
    p = C.RVQ_PROD
    codes = _rvq_run("prod_sem", p["n_q"], 0)
    _rvq_check(codes, "prod_sem", 0)
    assert (codes[:, 1:] == C.CODE_SENT).all()
    sem = codes[:, 0].copy()
    codes = _rvq_run("prod_ac", p["n_q"], p["n_sem"], codes)
    _rvq_check(codes, "prod_ac", p["n_sem"])
    assert (codes[:, 0] == sem).all()


# ---------------------------------------------------------------- mel front end and its tables
@pytest.fixture(scope="module")
def enc():
    e = q.SpeakerEncoder.from_synthetic(q.tiny_speaker_config())
    yield e
    e.close()


@pytest.fixture(scope="module")
def tables(enc):
    win, fb = enc.tables()
    win.setflags(write=False); fb.setflags(write=False)
    return win, fb


def test_tables(tables):
    win, fb = tables
    dw = float(np.abs(win.astype(np.float64) - C.hann64()).max())
    print(f"win: max |win - hann64| = {dw:.3e} = {dw / 2.0 ** -23:.2f} ulp(1) (bound 2)")
    assert dw <= 2 * 2.0 ** -23
    ref = C.slaney_fb64()
    dfb = float(np.abs(fb - ref).max())
    print(f"fb: max |fb - slaney64| = {dfb:.3e} = {dfb / (2e-3 * ref.max()):.3f} of the bound 2e-3 max(ref)")
    assert fb.shape == (128, 513) and (fb >= 0).all() and (fb.sum(1) > 0).all() and dfb <= 2e-3 * ref.max()
    ofb = O.mel_filterbank(24000, 1024, 128, 0.0, 12000.0)
    u = C.ulp_diff(fb, ofb)
    print(f"fb against the oracle's table: {u} ulp at most, bit-equal: {_same_bits(fb, ofb)}; win bit-equal to the oracle's: {_same_bits(win, O.hann_window(1024))}")
    assert u <= 1


@pytest.mark.parametrize("name,n", C.MEL_CASES)
def test_mel_against_f64(enc, tables, name, n):
    x = C.mel_case(name)
    mel = enc.mel(x)
    assert mel.shape == (128, q.SpeakerEncoder.mel_frames(n)) == (128, C.mel_frames(n))
    assert np.isfinite(mel).all(), f"{name}: {(~np.isfinite(mel)).sum()} non-finite outputs"
    dev = float(np.abs(mel.astype(np.float64) - C.mel_ref64(x, *tables)).max())
    _record("k_spk_stft_mel", dev, C.D_REF_MEL)
    assert dev <= 4 * C.D_REF_MEL, f"{name}: {dev:.3e} > 4 * {C.D_REF_MEL:.2e}"


# ---------------------------------------------------------------- speaker reductions
@pytest.mark.parametrize("T", C.RED_T)
def test_mean(T):
    x = C.red_case(T)
    buf, sl = _guarded(C.RED_C)
    q.spk_op_ex(SPK_MEAN, x, buf, C=C.RED_C, T=T, out_front=GUARD)
    assert np.isfinite(buf[sl]).all() and _guards_kept(buf, C.RED_C)
    dev = C.rel_dev(buf[sl], C.mean_ref(x))
    _record("k_spk_mean", dev, C.D_REF_MEAN)
    assert dev <= 4 * C.D_REF_MEAN, f"T={T}: {dev:.3e} > 4 * {C.D_REF_MEAN:.2e}"


@pytest.mark.parametrize("T", C.RED_T)
def test_asp_in(T):
    """rows [x ; mean ; std] judged separately; channel 1 is constant (std = sqrt(1e-5)), channel 2 = 1000 + 0.01 N(0, 1)"""
    x = C.red_case(T)
    n = 3 * C.RED_C * T
    buf, sl = _guarded(n)
    q.spk_op_ex(SPK_ASP_IN, x, buf, C=C.RED_C, T=T, out_front=GUARD)
    assert np.isfinite(buf[sl]).all() and _guards_kept(buf, n)
    got = buf[sl].reshape(3, C.RED_C, T)
    x64, mean64, std64 = C.asp_in_ref(x)
    assert _same_bits(got[0], x)                                                         # the x rows are a copy
    assert (got[1] == got[1][:, :1]).all() and (got[2] == got[2][:, :1]).all()           # one mean, one std per channel, broadcast over time
    for grp, got_g, ref in (("mean", got[1][:, 0], mean64), ("std", got[2][:, 0], std64)):
        dev = C.rel_dev(got_g, ref)
        _record(f"k_spk_asp_in {grp}", dev, C.D_REF_ASP_IN)
        assert dev <= 4 * C.D_REF_ASP_IN, f"T={T} {grp}: {dev:.3e} > 4 * {C.D_REF_ASP_IN:.2e}"


@pytest.mark.parametrize("name,T", C.POOL_CASES)
def test_asp_pool(name, T):
    aw, m = C.pool_case(name, T)
    n = 2 * C.RED_C
    buf, sl = _guarded(n)
    q.spk_op_ex(SPK_ASP_POOL, aw, buf, C=C.RED_C, T=T, b=m, out_front=GUARD)
    assert np.isfinite(buf[sl]).all() and _guards_kept(buf, n)
    got = buf[sl].reshape(2, C.RED_C)
    for grp, got_g, ref in zip(("mean", "std"), got, C.asp_pool_ref(aw, m)):
        dev = C.rel_dev(got_g, ref)
        _record(f"k_spk_asp_pool {grp}", dev, C.D_REF_ASP_POOL)
        assert dev <= 4 * C.D_REF_ASP_POOL, f"{name} T={T} {grp}: {dev:.3e} > 4 * {C.D_REF_ASP_POOL:.2e}"
    if name == "uniform":                                                               # equal logits: the plain mean, within the same bound
        plain = m.astype(np.float64).mean(axis=1)
        assert C.rel_dev(got[0], plain) <= 4 * C.D_REF_ASP_POOL


# ---------------------------------------------------------------- speaker movers
@pytest.mark.parametrize("with_b", [False, True], ids=["a", "a+b"])
@pytest.mark.parametrize("T,pl,pr", C.PAD_CASES)
def test_pad(T, pl, pr, with_b):
    a, b, _ = C.pad_case(T, pl, pr)
    Tp = T + pl + pr
    n = C.MOVE_C * Tp
    buf, sl = _guarded(n)
    q.spk_op_ex(SPK_PAD, a, buf, C=C.MOVE_C, T=T, pl=pl, Tp=Tp, b=b if with_b else None, out_front=GUARD)
    want = C.pad_ref(a, b if with_b else None, pl, pr)
    got = buf[sl].reshape(C.MOVE_C, Tp)
    assert _same_bits(got, want), f"T={T} pl={pl} pr={pr}: {(_bits(got) != _bits(want)).sum()} elements differ"
    assert _guards_kept(buf, n)


@pytest.mark.parametrize("T,pl,pr", C.PAD_CASES)
def test_cols(T, pl, pr):
    _, _, src = C.pad_case(T, pl, pr)
    tot = pl + pr
    n = C.MOVE_C * T
    buf, sl = _guarded(n)
    q.spk_op_ex(SPK_COLS, src, buf, C=C.MOVE_C, T=T, ld=T + tot, off=tot, out_front=GUARD)
    assert _same_bits(buf[sl].reshape(C.MOVE_C, T), np.ascontiguousarray(src[:, tot:])) and _guards_kept(buf, n)


@pytest.mark.parametrize("T", C.SE_T)
def test_se_apply(T):
    o, g, h = C.se_case(T)
    n = C.MOVE_C * T
    buf, sl = _guarded(n)
    buf[sl] = h.ravel()
    q.spk_op_ex(SPK_SE_APPLY, o, buf, C=C.MOVE_C, T=T, b=g, out_front=GUARD)
    assert _same_bits(buf[sl].reshape(C.MOVE_C, T), C.se_ref(o, g, h)) and _guards_kept(buf, n)


# ---------------------------------------------------------------- speech-encoder movers
@pytest.mark.parametrize("elu", [False, True], ids=["plain", "elu"])
@pytest.mark.parametrize("L,r", C.FOLD_PLAIN)
def test_fold_plain(L, r, elu):
    x = C.fold_case(L)
    Lf = C.fold_lf(L, r)
    n = C.FOLD_C * r * Lf
    buf, sl = _guarded(n)
    q.mimi_op_ex(MIMI_FOLD, x, buf, L=L, C=C.FOLD_C, r=r, Lf=Lf, elu=elu, out_front=GUARD)
    got = buf[sl].reshape(C.FOLD_C * r, Lf)
    assert _guards_kept(buf, n)
    if not elu:
        assert _same_bits(got, C.fold_ref(x, r, Lf))
        return
    assert np.isfinite(got).all()
    moved = C.fold_ref(x, r, Lf)
    assert _same_bits(got[moved > 0], moved[moved > 0])                                  # ELU is the identity on positive samples
    dev = C.rel_dev(got, C.fold_ref(x, r, Lf, elu=True, dtype=np.float64))
    _record("k_mimi_fold elu", dev, C.D_REF_ELU)
    assert dev <= 4 * C.D_REF_ELU, f"L={L} r={r}: {dev:.3e} > 4 * {C.D_REF_ELU:.2e}"


@pytest.mark.parametrize("L,Lf", C.FOLD_REPL)
def test_fold_replicate(L, Lf):
    x = C.fold_case(L)
    n = C.FOLD_C * 2 * (Lf + 1)
    buf, sl = _guarded(n)
    q.mimi_op_ex(MIMI_FOLD, x, buf, L=L, C=C.FOLD_C, r=2, Lf=Lf, replicate=True, out_front=GUARD)
    got = buf[sl].reshape(C.FOLD_C * 2, Lf + 1)
    assert _same_bits(got, C.fold_ref(x, 2, Lf, replicate=True)) and _guards_kept(buf, n)
    assert _same_bits(got[:, 0], np.repeat(x[:, 0], 2))                                  # the leading replicate column
    if 2 * Lf > L:
        assert _same_bits(got[1::2, -1], np.ascontiguousarray(x[:, L - 1]))              # the repeat of x[L - 1]


@pytest.mark.parametrize("n", C.ELU_N)
def test_elu(n):
    x = C.elu_case(n)
    buf, sl = _guarded(n)
    q.mimi_op_ex(MIMI_ELU, x, buf, L=n, out_front=GUARD)
    assert np.isfinite(buf[sl]).all() and _guards_kept(buf, n)
    assert _same_bits(buf[sl][x > 0], x[x > 0])
    dev = C.rel_dev(buf[sl], C.elu_ref(x))
    _record("k_mimi_elu", dev, C.D_REF_ELU)
    assert dev <= 4 * C.D_REF_ELU, f"n={n}: {dev:.3e} > 4 * {C.D_REF_ELU:.2e}"


@pytest.mark.parametrize("dim", C.CODEBOOK_DIMS)
def test_codebook(dim):
    esum, usage, want = C.codebook_case(dim)
    n = want.size
    buf, sl = _guarded(n)
    q.mimi_op_ex(MIMI_CODEBOOK, esum, buf, L=dim, C=len(C.CODEBOOK_USAGE), b=usage, out_front=GUARD)
    got = buf[sl].reshape(want.shape)
    assert np.isfinite(got).all() and _guards_kept(buf, n)
    u = C.ulp_diff(got, want)
    print(f"k_mimi_codebook dim={dim}: {u} ulp from numpy float32 at most")
    assert u <= 1
    assert _same_bits(got, want)          # measured 0 ulp on the MI355X at every dim: the division is correctly rounded
