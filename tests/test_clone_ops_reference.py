"""What tests/test_gpu_clone_ops.py rests on and a CPU can check: the float32 restatement of the quantiser against plain loops and
against float64, the tie case's own claims, the mel definition against the restatement of test_speaker_encoder.py, the float64
references of the pooling and the fold against plain loops, the frozen D_REF figures, and the refusal of every bad shape by the new
entry points before anything is launched."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
import clone_ops_cases as C
import oracle as O

INVALID = 1


# ---------------------------------------------------------------- residual vector quantiser
def test_rvq_f32_against_plain_loops():
    rng = np.random.default_rng(1)
    proj = rng.standard_normal((5, 4)).astype(np.float32)
    books = rng.standard_normal((3, 9, 5)).astype(np.float32)
    books[0, 6] = books[0, 2]; proj[:, 1] = books[0, 2]                 # an exact tie: the first minimum
    codes, resid = C.rvq_f32(proj, books)
    assert (codes == C.rvq_naive(proj, books)).all() and codes[1, 0] == 2
    assert len(resid) == 3 and all(r.dtype == np.float32 and r.shape == (4, 5) for r in resid)
    assert (resid[0] == proj.T).all() and (resid[1] == proj.T - books[0, codes[:, 0]]).all()


@pytest.mark.parametrize("name", C.RVQ_FLOAT_NAMES)
def test_rvq_f32_pick_is_a_float64_minimum_within_rounding(name):
    """the entry rvq_f32 picks at each layer is, in float64 on the same (float32) residual, within 1 + 2 (CD + 3) 2^-24 of the float64
    minimum: a float32 distance carries CD + 2 roundings of relative size 2^-24 at most on non-negative terms (the difference doubles
    in the square, the product, CD - 1 sums: no more than CD + 3 in all, first order), for the pick and for the true minimum alike"""
    proj, books = C.rvq_float_case(name)
    codes, resid = C.rvq_expected(name)
    CD = books.shape[2]
    bound = 1.0 + 2.0 * (CD + 3) * 2.0 ** -24
    bk = books.astype(np.float64)
    worst = 1.0
    for l, r in enumerate(resid):
        d = ((r.astype(np.float64)[:, None, :] - bk[l][None]) ** 2).sum(axis=2)           # [T][CB]
        picked = d[np.arange(d.shape[0]), codes[:, l]]
        assert (picked <= d.min(axis=1) * bound).all(), (name, l)
        worst = max(worst, float((picked / d.min(axis=1)).max()))
    print(f"{name}: worst picked / minimum = 1 + {worst - 1.0:.2e} (bound 1 + {bound - 1.0:.2e})")


def test_rvq_ties_case_is_what_it_claims():
    c = C.TIES
    proj, books = C.rvq_ties_case()
    assert proj.shape == (c["CD"], c["T"]) and books.shape == (c["n_layers"], c["CB"], c["CD"])
    for a in (proj, books):
        assert (a == np.round(a)).all() and np.abs(a).max() <= 2
    assert c["CB"] - 2 * 256 == 88                                                          # threads 0..87 own three entries
    codes32, _ = C.rvq_f32(proj, books); codes64, _ = C.rvq_f64(proj, books)
    assert (codes32 == codes64).all()
    d0 = ((proj.T[:, None, :] - books[0][None]) ** 2).sum(axis=2)                          # exact in float32
    for i, (lo, hi) in enumerate(C.TIES_PAIRS):
        assert lo < hi and (books[0, lo] == books[0, hi]).all()
        assert sorted(np.flatnonzero(d0[i] == 0)) == [lo, hi] and codes32[i, 0] == lo     # the tie is the minimum; the lower index wins
    (a, b), (a2, b2), (a3, b3), (a4, b4) = C.TIES_PAIRS
    assert a % 256 == b % 256                                                              # one thread
    assert b2 - a2 == 128 and a2 < 128 and a3 < 128 <= b3 < 256                             # first reduction step: tid and tid + 128 / the two halves
    assert a4 < 256 <= b4 and a4 % 256 != b4 % 256                                          # different strides, different threads
    # the pair whose lower index sits in the higher thread, alone at distance 0 on its own frame
    lo, hi = C.TIES_HIGH_THREAD
    f = C.TIES_OWN_FRAME
    assert lo < hi and lo % 256 > hi % 256
    assert list(np.flatnonzero(d0[f] == 0)) == [C.TIES_OWN_ENTRY] and codes32[f, 0] == C.TIES_OWN_ENTRY
    r1 = proj.T[f] - books[0, codes32[f, 0]]
    d1 = ((r1[None, :] - books[1]) ** 2).sum(axis=1)
    assert not r1.any() and list(np.flatnonzero(d1 == 0)) == [lo, hi] and codes32[f, 1] == lo
    assert all(codes32[i, 1] == lo for i in range(len(C.TIES_PAIRS)))                      # the pair frames meet the same tie


def test_rvq_float_cases_reach_what_they_name():
    assert [(CB, CD) for _, CB, CD, _, _ in C.RVQ_SMALL] == [(64, 24), (2, 1), (300, 255)]
    cfg = q.tiny_speech_config()
    assert (cfg.cb_size, cfg.cb_dim) == (64, 24)
    p = C.RVQ_PROD
    assert C.rvq_float_case("prod_sem")[1].shape == (1, 2048, 256) and C.rvq_float_case("prod_ac")[1].shape == (15, 2048, 256)
    assert p["n_q"] == 16 and C.rvq_float_case("prod_ac")[0].shape == (256, 3)


# ---------------------------------------------------------------- mel
def _tables32():
    return O.hann_window(1024), O.mel_filterbank(24000, 1024, 128, 0.0, 12000.0)


def test_mel_ref64_against_the_numpy_restatement():
    """a long clip, where no clamp fires and the reflect rule is np.pad's: the restatement of
    test_speaker_encoder.py::test_mel_frame_count_and_values (float64 Hann, rfft, the oracle's filterbank)"""
    rng = np.random.default_rng(1)
    x = (0.2 * rng.standard_normal(12000)).astype(np.float32)
    win = C.hann64(); fb = _tables32()[1]
    xp = np.pad(x.astype(np.float64), 384, mode="reflect")
    T = (len(xp) - 1024) // 256 + 1
    fr = np.stack([xp[i * 256:i * 256 + 1024] * win for i in range(T)])
    mag = np.sqrt(np.abs(np.fft.rfft(fr, axis=1)) ** 2 + 1e-9)
    ref = np.log(np.maximum(mag @ fb.astype(np.float64).T, 1e-5)).T
    got = C.mel_ref64(x, win, fb)
    assert got.shape == ref.shape == (128, C.mel_frames(12000)) and np.abs(got - ref).max() < 1e-10
    # and the oracle's float32 front end agrees with it to its own tolerance
    assert np.abs(O.mel_speaker(x) - C.mel_ref64(x, *_tables32())).max() < 2e-3


def test_mel_cases_reach_what_they_name():
    assert [C.mel_frames(n) for _, n in C.MEL_CASES] == [q.SpeakerEncoder.mel_frames(n) for _, n in C.MEL_CASES] == [1, 1, 1, 1, 2, 4, 19, 8, 8]
    fired = {}
    for n in (256, 300, 384, 385):
        idx = C.mel_index(n)
        p = np.arange(1024) - 384
        left = (p < 0) & (-p >= n); right = (p >= n) & (n < 2 + (p - n))
        fired[n] = (int(left.sum()), int(right.sum()))
        assert idx.min() >= 0 and idx.max() < n
        assert (idx[0][left] == n - 1).all() and (idx[0][right] == 0).all()
    assert fired[256][0] > 0 and fired[256][1] > 0 and fired[384] == (1, 0) and fired[385] == (0, 0) and fired[300][0] > 0
    # where no clamp fires the rule is plain reflection
    x = np.arange(5000, dtype=np.float64)
    assert (x[C.mel_index(5000)][0] == np.pad(x, 384, mode="reflect")[:1024]).all()
    assert (x[C.mel_index(5000)][-1] == np.pad(x, 384, mode="reflect")[18 * 256:18 * 256 + 1024]).all()
    win, fb = _tables32()
    assert (C.mel_ref64(C.mel_case("silence"), win, fb) == np.log(1e-5)).all()               # every band at the floor
    s = C.mel_ref64(C.mel_case("sine"), win, fb)
    assert s.max() > 0 and (s[:, 3] == np.log(1e-5)).sum() > 64                              # a peak, and most bands of an inner frame at the floor


def test_table_references():
    """the float64 tables the GPU's are held to, against the oracle's float32 ones"""
    win, fb = _tables32()
    assert np.abs(win.astype(np.float64) - C.hann64()).max() <= 2 * 2.0 ** -23              # 2 ulp(1): cosf of a float32 argument
    ref = C.slaney_fb64()
    assert np.abs(fb - ref).max() <= 2e-3 * ref.max()                                        # test_mel_filterbank_properties' bound


# ---------------------------------------------------------------- reductions, fold
def test_asp_pool_reference_against_plain_loops():
    rng = np.random.default_rng(2)
    aw = rng.standard_normal((2, 7)).astype(np.float32) * 3; m = rng.standard_normal((2, 7)).astype(np.float32)
    for got, want in zip(C.asp_pool_ref(aw, m), C.asp_pool_naive(aw, m)):
        assert np.abs(got - want).max() < 1e-13
    wm, ws = C.asp_pool_ref(*C.pool_case("uniform", 513))
    m = C.pool_case("uniform", 513)[1].astype(np.float64)
    assert np.abs(wm - m.mean(axis=1)).max() < 1e-14 and np.abs(ws - np.sqrt(m.var(axis=1) + 1e-5)).max() < 1e-14
    aw, m = C.pool_case("hot", C.POOL_HOT_T)
    wm, ws = C.asp_pool_ref(aw, m)
    assert (np.sort(aw, axis=1)[:, -1] - np.sort(aw, axis=1)[:, -2] == C.POOL_HOT).all()
    assert np.abs(wm - m[:, C.POOL_HOT_AT]).max() < 1e-30 and np.abs(ws - np.sqrt(1e-5)).max() < 1e-30
    aw, _ = C.pool_case("deep", 257)
    assert aw.max() < -9.9e3 and np.ptp(aw) > 1.0
    x, mean, std = C.asp_in_ref(C.red_case(257))
    assert mean[1] == C.CONST_VALUE and std[1] == np.sqrt(1e-5) and abs(mean[2] - 1000) < 0.01 and 0.005 < std[2] < 0.02
    for T in C.RED_T:
        assert C.red_case(T).shape == (C.RED_C, T)


def test_fold_reference_against_plain_loops():
    for (L, r) in C.FOLD_PLAIN:
        x = C.fold_case(L); Lf = C.fold_lf(L, r)
        assert (Lf - 1) * r < L <= Lf * r
        y = C.fold_ref(x, r, Lf)
        assert y.dtype == np.float32 and y.shape == (C.FOLD_C * r, Lf) and (y == C.fold_naive(x, r, Lf)).all()
    for (L, Lf) in C.FOLD_REPL:
        x = C.fold_case(L)
        y = C.fold_ref(x, 2, Lf, replicate=True)
        assert y.shape == (C.FOLD_C * 2, Lf + 1) and (y == C.fold_naive(x, 2, Lf, replicate=True)).all()
        assert (y[:, 0] == np.repeat(x[:, 0], 2)).all()                                     # the leading replicate column, both phases
        if 2 * Lf > L:
            assert (y[1::2, -1] == x[:, L - 1]).all()                                       # the repeat of the last sample
    x = C.fold_case(7)
    e64 = C.fold_ref(x, 3, 3, elu=True, dtype=np.float64)
    assert e64.dtype == np.float64 and np.abs(e64 - np.where(C.fold_naive(x, 3, 3) > 0, C.fold_naive(x, 3, 3), np.expm1(C.fold_naive(x, 3, 3).astype(np.float64)))).max() == 0
    for n in C.ELU_N:
        v = C.elu_case(n)
        assert (v <= 0).any() and (n <= 2 or (v[1] == 0.0 and v[2] == np.float32(-1e-6)))
    for T, pl, pr in C.PAD_CASES:
        assert 0 <= pl <= T - 1 and 0 <= pr <= T - 1 and pl == (pl + pr) // 2
        a, b, src = C.pad_case(T, pl, pr)
        assert C.pad_ref(a, b, pl, pr).shape == src.shape == (C.MOVE_C, T + pl + pr) and C.pad_ref(a, None, pl, pr).dtype == np.float32
    assert C.pad_ref(np.arange(5, dtype=np.float32)[None], None, 2, 2).tolist() == [[2, 1, 0, 1, 2, 3, 4, 3, 2]]      # speaker.rs:412-452


# ---------------------------------------------------------------- D_REF
def test_d_ref_is_what_numpy_float32_gives():
    """the frozen constants are the measured worst case of the references in numpy float32: each measurement lies within
    [0.5, 1.0] x its constant — neither exceeded nor padded"""
    d = C.d_ref_reductions()
    d["mel"] = C.d_ref_mel(*_tables32())
    consts = {"mel": C.D_REF_MEL, "mean": C.D_REF_MEAN, "asp_in": C.D_REF_ASP_IN, "asp_pool": C.D_REF_ASP_POOL, "elu": C.D_REF_ELU}
    print({k: f"{v:.3e}" for k, v in d.items()})
    for k, c in consts.items():
        assert 0.5 * c <= d[k] <= c, (k, d[k], c)
    assert 4 * C.D_REF_MEL <= 1e-5 and 4 * max(C.D_REF_MEAN, C.D_REF_ASP_IN, C.D_REF_ASP_POOL, C.D_REF_ELU) <= 2e-6


def test_codebook_and_ulp_helper():
    assert C.ulp_diff(np.float32([1.0, -1.0]), np.float32([1.0, -1.0])) == 0
    assert C.ulp_diff(np.float32([1.0]), np.nextafter(np.float32([1.0]), np.float32(2))) == 1
    assert C.ulp_diff(np.float32([-0.0]), np.float32([0.0])) == 0 and C.ulp_diff(np.float32([1e-45]), np.float32([-1e-45])) == 2
    for dim in C.CODEBOOK_DIMS:
        esum, usage, exp = C.codebook_case(dim)
        assert exp.dtype == np.float32 and exp.shape == (6, dim) and np.isfinite(exp).all()
        for e in (0, 1, 2):                                                                  # at or below the clamp: divided by 1e-5
            assert (exp[e] == esum[e] / np.float32(1e-5)).all()
        assert (exp[3] == esum[3] / np.float32(0.5)).all() and (exp[5] == esum[5] / np.float32(1e4)).all()


# ---------------------------------------------------------------- refusals
def _refused(call, what):
    with pytest.raises(_lib.Q3Error) as e:
        call()
    assert e.value.status == INVALID, f"{what}: status {e.value.status} ({e.value})"
    assert len(str(e.value)) > len("q3 status 1: "), what


def test_entry_points_refuse_bad_shapes_before_launching():
    """Q3_INVALID_ARG with a message — not a HIP error, not a launch — for every shape the kernels could not address; checked before the
    device is touched, so it holds on a machine without a GPU"""
    z = lambda *s: np.zeros(s, np.float32)
    assert ctypes.sizeof(_lib.CSpkOpEx) == 8 * 4 + 4 * 8 + 3 * 8 and ctypes.sizeof(_lib.CMimiOpEx) == 8 * 4 + 4 * 8 + 3 * 8
    # RVQ
    rvq = lambda CD=8, CB=4, nl=2, T=3, n_q=4, q0=0: q.mimi_rvq_ex(z(CD, T), z(nl, CB, CD), np.zeros((T, n_q), np.uint32), q0=q0)
    _refused(lambda: rvq(CD=257), "CD > 256")
    _refused(lambda: rvq(CD=0), "CD < 1")
    _refused(lambda: rvq(CB=0), "CB < 1")
    _refused(lambda: rvq(nl=0), "n_layers < 1")
    _refused(lambda: rvq(q0=-1), "q0 < 0")
    _refused(lambda: rvq(nl=2, n_q=4, q0=3), "q0 + n_layers > n_q")
    _refused(lambda: rvq(T=0), "T < 1")
    _refused(lambda: q.mimi_rvq_ex(np.full((8, 3), np.inf, np.float32), z(2, 4, 8), np.zeros((3, 4), np.uint32)), "a frame without a finite distance")
    # pad
    pad = lambda T, pl, Tp, C=2, b=False: q.spk_op_ex(q.api.SPK_PAD, z(C, T), z(C * max(Tp, 1)), C=C, T=T, pl=pl, Tp=Tp, b=z(C, T) if b else None)
    _refused(lambda: pad(5, -1, 6), "pl < 0")
    _refused(lambda: pad(5, 2, 6), "Tp < T + pl")
    _refused(lambda: pad(5, 5, 12), "pl > T - 1")
    _refused(lambda: pad(5, 1, 11), "right pad > T - 1")
    _refused(lambda: pad(1, 1, 3), "T = 1 cannot be padded")
    _refused(lambda: q.spk_op_ex(q.api.SPK_PAD, z(2, 5), z(2 * 9 - 1), C=2, T=5, pl=2, Tp=9), "out too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_PAD, z(2, 5), z(2 * 9 + 3), C=2, T=5, pl=2, Tp=9, out_front=4), "out_front pushes the result out")
    _refused(lambda: q.spk_op_ex(q.api.SPK_PAD, z(2, 4), z(2 * 9), C=2, T=5, pl=2, Tp=9), "a too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_PAD, z(2, 5), z(2 * 9), C=2, T=5, pl=2, Tp=9, b=z(2, 4)), "b too small")
    # cols
    cols = lambda T, ld, off, C=2: q.spk_op_ex(q.api.SPK_COLS, z(C, max(ld, 1)), z(C * max(T, 1)), C=C, T=T, ld=ld, off=off)
    _refused(lambda: cols(5, 8, 4), "off + T > ld")
    _refused(lambda: cols(5, 8, -1), "off < 0")
    _refused(lambda: cols(0, 8, 0), "T < 1")
    # reductions and SE
    for op, name in ((q.api.SPK_MEAN, "mean"), (q.api.SPK_ASP_IN, "asp_in")):
        _refused(lambda: q.spk_op_ex(op, z(2, 5), z(64), C=2, T=0), f"{name}: T < 1")
        _refused(lambda: q.spk_op_ex(op, z(2, 5), z(64), C=0, T=5), f"{name}: C < 1")
        _refused(lambda: q.spk_op_ex(op, z(2, 4), z(64), C=2, T=5), f"{name}: a too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_MEAN, z(2, 5), z(1), C=2, T=5), "mean: out too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_ASP_IN, z(2, 5), z(29), C=2, T=5), "asp_in: out too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_ASP_POOL, z(2, 5), z(4), C=2, T=0, b=z(2, 5)), "asp_pool: T < 1")
    _refused(lambda: q.spk_op_ex(q.api.SPK_ASP_POOL, z(2, 5), z(4), C=0, T=5, b=z(2, 5)), "asp_pool: C < 1")
    _refused(lambda: q.spk_op_ex(q.api.SPK_ASP_POOL, z(2, 5), z(4), C=2, T=5), "asp_pool: no m")
    _refused(lambda: q.spk_op_ex(q.api.SPK_ASP_POOL, z(2, 5), z(3), C=2, T=5, b=z(2, 5)), "asp_pool: out too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_SE_APPLY, z(2, 5), z(10), C=2, T=5, b=z(1)), "se_apply: g too small")
    _refused(lambda: q.spk_op_ex(q.api.SPK_SE_APPLY, z(2, 5), z(10), C=2, T=0, b=z(2)), "se_apply: T < 1")
    _refused(lambda: q.spk_op_ex(6, z(2, 5), z(10), C=2, T=5), "op 6")
    # fold
    fold = lambda L, r, Lf, C=2, rep=False, out=None: q.mimi_op_ex(q.api.MIMI_FOLD, z(C, max(L, 1)), z(4096) if out is None else out, L=L, C=C, r=r, Lf=Lf,
                                                                 replicate=rep)
    _refused(lambda: fold(7, 0, 3), "r < 1")
    _refused(lambda: fold(0, 2, 3), "L < 1")
    _refused(lambda: fold(7, 2, 0), "Lf < 1")
    _refused(lambda: fold(7, 3, 4), "plain: (Lf - 1) * r >= L")
    _refused(lambda: fold(6, 3, 3), "plain: (Lf - 1) * r == L")
    _refused(lambda: fold(7, 2, 4, out=z(2 * 2 * 4 - 1)), "fold: out too small")
    _refused(lambda: fold(7, 2, 4, rep=True, out=z(2 * 2 * 5 - 1)), "replicate fold: out too small (the leading column)")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_FOLD, z(2, 6), z(4096), L=7, C=2, r=2, Lf=4), "fold: a too small")
    # ELU, codebook
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_ELU, z(8), z(7), L=8), "elu: out too small")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_ELU, z(7), z(8), L=8), "elu: a too small")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_ELU, z(8), z(8), L=0), "elu: n < 1")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_CODEBOOK, z(6, 24), z(6 * 24), L=24, C=6), "codebook: no usage")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_CODEBOOK, z(6, 24), z(6 * 24), L=24, C=6, b=z(5)), "codebook: usage too small")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_CODEBOOK, z(6, 24), z(6 * 24), L=0, C=6, b=z(6)), "codebook: dim < 1")
    _refused(lambda: q.mimi_op_ex(q.api.MIMI_CODEBOOK, z(6, 24), z(6 * 24), L=24, C=0, b=z(6)), "codebook: no entries")
    _refused(lambda: q.mimi_op_ex(3, z(8), z(8), L=8), "op 3")
    # tables: a handle without a device has none
    enc = q.SpeakerEncoder(q.tiny_speaker_config(), device=-1)
    _refused(enc.tables, "tables of a manifest-only handle")
    enc.close()
    st = _lib.lib.q3_spk_tables(None, None, None)
    assert st == INVALID and len(_lib.lib.q3_last_error()) > 0


def test_mel_frames_out_of_range():
    """q3_spk_mel_frames: 0 for a clip too short for a frame (negative counts included), the closed form up to 2^38 samples, -1 (no
    count) above — it used to add 768 to any n_samples, a signed overflow near INT64_MAX, and to truncate the count long before."""
    f = _lib.lib.q3_spk_mel_frames
    assert [f(n) for n in (-(1 << 63), -1, 0, 1, 255)] == [0] * 5
    assert [f(n) for n in (256, 511, 512, 24000 * 120)] == [1, 1, 2, (24000 * 120 + 768 - 1024) // 256 + 1]
    assert f(1 << 38) == ((1 << 38) + 768 - 1024) // 256 + 1 == (1 << 30)
    assert [f(n) for n in ((1 << 38) + 1, 1 << 40, (1 << 63) - 768, (1 << 63) - 6, (1 << 63) - 1)] == [-1] * 5
