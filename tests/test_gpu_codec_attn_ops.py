"""Op-level tests of the codec transformer's [C][L] kernels (-m gpu): one launch at a time against float64 numpy. Inputs, case
tables (each names what it reaches) and references live in codec_attn_cases.py; what needs no GPU — the D_REF recomputation, the
reference against plain loops, the refusal of bad shapes, the host-only kernel selection — is in test_codec_attn_reference.py.

Attention (q3_attn_c_ex -> ONE launch_attn_c with k_attn_c or k_attn_c_mfma, launch_attn_cs, launch_attn_cb, launch_mimi_attn).
The measure is max |o - o64| / max |o64| per case, the bound 4 * D_REF (the rule of test_gpu_attention_op.py: the same reference in
numpy float32 deviates from f64 by at most D_REF over this file's cases; two for another summation order, two for a fast exp); the
stress cases have D_REF_STRESS, their own by the same rule. `o` goes in filled with a NaN of known bits: every element a launch owns
must be finite, every other one must keep those bits. The stream caches are NaN at and beyond each row's end, in the whole other
layer, in the unowned blocks: one such value read into an MFMA turns 0 x NaN into a NaN result.
Bit-identity, as the code promises (a query's arithmetic depends only on its absolute index): k_attn_cs / k_attn_cb rows equal
columns [a0, e) of k_attn_c_mfma over the same K / V at L = e; k_attn_c_mfma at L = 129 equals its L = 97 run on the first 97
columns; queries in front of a stress case's hot key equal the case without it.

RoPE equals numpy float32 with separately rounded products and sum bit for bit; the movers and k_rvq_embed are bit-exact with
sentinels around every destination; k_silu_mul is held to 4 x what numpy float32 deviates from f64 on the same formula.

Measured on an MI355X (worst over every case of this file, in units of the case's D_REF; bound 4; each test prints its own with -s):
  k_attn_c_mfma 0.34 (stress 0.60), k_attn_c 0.33 (stress 0.56), k_attn_cs 0.55, k_attn_cb 0.67, k_mimi_attn 0.36, k_silu_mul 0.84
No kernel missed a check."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import codec_attn_cases as C
from codec_attn_cases import HD, NH, QD, VALU, MFMA, D_REF, D_REF_STRESS, D_REF_SILU

pytestmark = pytest.mark.gpu

assert "Q3_ATTN_C_VALU" not in os.environ, "Q3_ATTN_C_VALU set: the engine's pick would not be the kernel the cases name"

WORST = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and (_bits(a) == _bits(b)).all()


def _record(name, dev, d_ref):
    WORST[name] = max(WORST.get(name, 0.0), dev / d_ref)
    print(f"{name}: dev {dev:.3e} = {dev / d_ref:.2f} D_REF; worst so far {({k: round(v, 2) for k, v in WORST.items()})}")


@pytest.fixture(scope="module")
def whole():
    """k_attn_c_mfma / k_attn_c / engine's pick over a whole case, one launch per (kernel, case), shared by the tests"""
    cache = {}

    def run(L, nh, kernel, hot_key=None, seed=0):
        key = (L, nh, kernel, hot_key, seed)
        if key not in cache:
            qq, k, v = C.whole_case(L, nh, hot_key, seed)
            o = q.attn_c_ex(0, qq, C.sentinel(qq.shape), nh=nh, k=k, v=v, kernel=kernel)
            o.setflags(write=False)
            cache[key] = o
        return cache[key]
    return run


# ---------------------------------------------------------------- whole utterance
@pytest.mark.parametrize("kernel", [MFMA, VALU], ids=["mfma", "valu"])
@pytest.mark.parametrize("L,nh", C.WHOLE_CASES)
def test_whole_against_f64(whole, kernel, L, nh):
    o = whole(L, nh, kernel)
    assert np.isfinite(o).all(), f"L={L} nh={nh}: {(~np.isfinite(o)).sum()} non-finite outputs"
    dev = C.dev(o, C.whole_ref64(L, nh))
    _record("k_attn_c_mfma" if kernel == MFMA else "k_attn_c", dev, D_REF)
    assert dev <= 4 * D_REF, f"L={L} nh={nh} kernel={kernel}: {dev:.3e} > 4 * {D_REF:.2e}"


def test_engine_pick_is_the_mfma_kernel(whole):
    assert q.attn_c_path() == MFMA
    for (L, nh) in ((97, 2), (300, 2)):
        assert _same_bits(whole(L, nh, -1), whole(L, nh, MFMA))
    assert not _same_bits(whole(300, 2, VALU), whole(300, 2, MFMA))          # the explicit form ran another kernel, not the pick twice


@pytest.mark.parametrize("kernel", [MFMA, VALU], ids=["mfma", "valu"])
@pytest.mark.parametrize("hot_key", C.STRESS_KEYS)
def test_whole_softmax_stress(whole, kernel, hot_key):
    """a key ~60 logits above the rest in the tile of wave 0 / 1 / 3: the merge must carry a dominant tile from any wave"""
    L = C.STRESS_L
    o = whole(L, NH, kernel, hot_key)
    assert np.isfinite(o).all()
    dev = C.dev(o, C.whole_ref64(L, NH, hot_key))
    _record(("k_attn_c_mfma" if kernel == MFMA else "k_attn_c") + " stress", dev, D_REF_STRESS)
    assert dev <= 4 * D_REF_STRESS, f"hot key {hot_key} kernel={kernel}: {dev:.3e} > 4 * {D_REF_STRESS:.2e}"
    # queries in front of the hot key, and head 1 throughout, do not see it: the same bits as the case without it
    base = whole(L, NH, kernel)
    assert _same_bits(o[:, :hot_key], base[:, :hot_key]) and _same_bits(o[HD:], base[HD:])


def test_mfma_prefix_keeps_its_bits(whole):
    """k_attn_c_mfma at L = 129 over the data of which L = 97 is a prefix: the first 97 columns are bit-equal"""
    q129, k129, v129 = C.whole_case(129, NH)
    o129 = whole(129, NH, MFMA)
    cut = lambda a: np.ascontiguousarray(a[:, :97])
    o97 = q.attn_c_ex(0, cut(q129), C.sentinel((QD, 97)), nh=NH, k=cut(k129), v=cut(v129), kernel=MFMA)
    assert _same_bits(o129[:, :97], o97)


# ---------------------------------------------------------------- stream / blocked stream
def _check_rows(o, rows, qcols, name, whole):
    """every row: finite, within the f64 bound, bit-equal to k_attn_c_mfma at L = e; every other column keeps the sentinel"""
    owned = np.zeros(o.shape[1], dtype=bool)
    for (a0, e), c in zip(rows, qcols):
        n = e - a0
        got = o[:, c:c + n]
        owned[c:c + n] = True
        assert np.isfinite(got).all(), f"{name} row ({a0}, {e}): {(~np.isfinite(got)).sum()} non-finite outputs"
        dev = C.dev(got, C.row_ref64(a0, e))
        _record(name, dev, D_REF)
        assert dev <= 4 * D_REF, f"{name} row ({a0}, {e}): {dev:.3e} > 4 * {D_REF:.2e}"
        ref = whole(e, NH, MFMA, None, C.row_seed(a0, e))
        assert _same_bits(got, ref[:, a0:e]), f"{name} row ({a0}, {e}) differs from k_attn_c_mfma at L = {e}"
    assert C.is_sentinel(o[:, ~owned]).all(), f"{name}: columns outside the rows' new frames written"


@pytest.mark.parametrize("rows", [C.STREAM_ROWS, C.STREAM_SINGLE], ids=["four_rows", "single"])
def test_stream(whole, rows):
    N, qcols = C.stream_layout(rows)
    r3 = [(a0, e, c) for (a0, e), c in zip(rows, qcols)]
    o = q.attn_c_ex(1, C.stream_q(rows), C.sentinel((QD, N)), nh=NH, rows=r3, caches=C.stream_caches(rows), layer=C.LAYER)
    _check_rows(o, rows, qcols, "k_attn_cs", whole)


def test_stream_leaves_other_rows_columns_alone(whole):
    """a launch over rows 2 and 4 only, in the four rows' layout: the columns of rows 1 and 3 keep the sentinel too"""
    N, qcols = C.stream_layout(C.STREAM_ROWS)
    pick = (1, 3)
    rows = [C.STREAM_ROWS[i] for i in pick]; cols = [qcols[i] for i in pick]
    r3 = [(a0, e, c) for (a0, e), c in zip(rows, cols)]
    o = q.attn_c_ex(1, C.stream_q(C.STREAM_ROWS), C.sentinel((QD, N)), nh=NH, rows=r3, caches=C.stream_caches(rows), layer=C.LAYER)
    _check_rows(o, rows, cols, "k_attn_cs", whole)


@pytest.mark.parametrize("rows", [C.BLOCKED_ROWS, C.STREAM_SINGLE], ids=["four_rows", "single"])
@pytest.mark.parametrize("bf", C.BLOCK_FRAMES)
def test_blocked_stream(whole, bf, rows):
    N, qcols = C.stream_layout(rows)
    r3 = [(a0, e, c) for (a0, e), c in zip(rows, qcols)]
    pool, tabs, tab0, tab_n = C.blocked_pool(rows, bf)
    o = q.attn_c_ex(2, C.stream_q(rows), C.sentinel((QD, N)), nh=NH, rows=r3, caches=pool, layer=C.LAYER, tabs=tabs, tab0=tab0, tab_n=tab_n)
    _check_rows(o, rows, qcols, "k_attn_cb", whole)


# ---------------------------------------------------------------- sliding window
@pytest.mark.parametrize("T,window", C.WINDOW_CASES)
def test_window_against_f64(T, window):
    qq, k, v = C.whole_case(T, NH)
    o = q.attn_c_ex(3, qq, C.sentinel(qq.shape), nh=NH, k=k, v=v, window=window)
    assert np.isfinite(o).all()
    dev = C.dev(o, C.whole_ref64(T, NH, None, 0, window))
    _record("k_mimi_attn", dev, D_REF)
    assert dev <= 4 * D_REF, f"T={T} window={window}: {dev:.3e} > 4 * {D_REF:.2e}"


def test_window_covering_everything_is_causal_attention():
    qq, k, v = C.whole_case(C.WINDOW_T, NH)
    o = q.attn_c_ex(3, qq, C.sentinel(qq.shape), nh=NH, k=k, v=v, window=C.WINDOW_T + 5)
    dev = C.dev(o, C.whole_ref64(C.WINDOW_T, NH))
    _record("k_mimi_attn", dev, D_REF)
    assert np.isfinite(o).all() and dev <= 4 * D_REF


# ---------------------------------------------------------------- RoPE
@pytest.mark.parametrize("with_pos", [False, True], ids=["k_rope_c", "k_rope_c_pos"])
@pytest.mark.parametrize("L", C.ROPE_L)
def test_rope_bits(L, with_pos):
    cs, sn = C.rope_tables()
    x_q, x_k = C.rope_case(L)
    pos = C.rope_pos(L) if with_pos else np.arange(L, dtype=np.int32)
    got_q, got_k = q.rope_c_ex(x_q, x_k, cs, sn, NH, pos=pos if with_pos else None)
    for got, x, name in ((got_q, x_q, "q"), (got_k, x_k, "k")):
        want = C.rope_reference(x, pos)
        assert _same_bits(got, want), f"L={L} {name}: {(_bits(got) != _bits(want)).sum()} elements differ from separately rounded float32"
        assert _same_bits(got, x) == (not pos.any())          # position 0 is the identity; anything else rotates


# ---------------------------------------------------------------- movers
@pytest.mark.parametrize("Cc", C.COPY_COLS_C)
@pytest.mark.parametrize("n", C.COPY_COLS_N)
def test_copy_cols(n, Cc):
    src, dst, s_off, d_off, sp, dp, exp = C.copy_cols_case(n, Cc)
    got = q.copy_cols_ex(src, dst, Cc, s_off, d_off, sp, dp, src_off=C.COPY_COLS_OFF[0], dst_off=C.COPY_COLS_OFF[1])
    assert _same_bits(got, exp), f"n={n} C={Cc}: {(_bits(got) != _bits(exp)).sum()} elements differ (sentinels included)"


def test_copy_segs():
    src, dst, segs, exp = C.copy_segs_case()
    assert _same_bits(q.copy_segs_ex(src, dst, segs), exp)


@pytest.mark.parametrize("n", C.GATHER_N)
def test_gather_frames(n):
    src, s_off, dst, exp = C.gather_case(n)
    assert (q.gather_frames_ex(src, s_off, dst) == exp).all()


# ---------------------------------------------------------------- split-RVQ lookup, SiLU * u
@pytest.mark.parametrize("cb_dim,n_frames", C.RVQ_CASES)
def test_rvq_embed(cb_dim, n_frames):
    frames, fcb, rest, fo, ro = C.rvq_case(cb_dim, n_frames)
    n = cb_dim * n_frames
    first = C.sentinel(C.GUARD + n + C.GUARD); rest_out = C.sentinel(C.GUARD + n + C.GUARD)
    q.rvq_embed_ex(frames, fcb, rest, first, rest_out, out_front=C.GUARD)
    for got, want, name in ((first, fo, "first_out"), (rest_out, ro, "rest_out")):
        assert _same_bits(got[C.GUARD:C.GUARD + n].reshape(cb_dim, n_frames), want), f"{name} cb_dim={cb_dim} n_frames={n_frames}"
        assert C.is_sentinel(got[:C.GUARD]).all() and C.is_sentinel(got[C.GUARD + n:]).all(), f"{name}: guard written"


@pytest.mark.parametrize("n", C.SILU_N)
def test_silu_mul(n):
    g, u = C.silu_case(n)
    y = q.silu_mul_ex(g, u, C.sentinel(n + C.GUARD))
    assert C.is_sentinel(y[n:]).all() and np.isfinite(y[:n]).all()
    y64 = C.silu_reference(g, u)
    dev = float(np.abs(y[:n].astype(np.float64) - y64).max() / np.abs(y64).max())
    _record("k_silu_mul", dev, D_REF_SILU)
    assert dev <= 4 * D_REF_SILU, f"n={n}: {dev:.3e} > 4 * {D_REF_SILU:.2e}"
